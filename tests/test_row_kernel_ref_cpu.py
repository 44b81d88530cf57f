"""tests/_row_kernel_ref.py checked without a GPU: (1) every reference equals the oracle or autograd to 1e-12, (2) the bounds
admit an honest fp32 implementation (torch.float32, torch's summation order, output rounded to the dtype) on every shape and
input class, (3) every listed mutation of a reference output exceeds its bound, (4) the inputs have the properties the GPU
tests lean on."""
import math

import numpy as np
import pytest
import torch

import _row_kernel_ref as R
from oracle import dropout as DO
from oracle import whisper_oracle as O

F32, BF16, F64 = R.F32, R.BF16, R.F64
DTYPES = [F32, BF16]
U = R.U


def close(a, b, tol=1e-12):
    a, b = a.to(F64), b.to(F64)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def ulp_step(t, idx, dtype):
    """t[idx] moved by 1 bf16 ulp (bf16) or 64 fp32 ulps (fp32), upwards in magnitude."""
    t = t.clone()
    v = float(t[idx])
    if dtype == BF16:
        b = torch.tensor([v], dtype=F32).to(BF16).view(torch.int16)
        t[idx] = float((b + 1).view(BF16).float())
    else:
        b = torch.tensor([v], dtype=F32).view(torch.int32)
        t[idx] = float((b + 64).view(F32))
    return t


def ln_keep(inp, seed_off=0):
    keep = torch.from_numpy(DO.keep_flat(R.LN_DROP_SEED + seed_off, inp["rows"], inp["C"], R.LN_DROP_P))
    return keep, DO.keep_scale(R.LN_DROP_P)


def ln_all_cases():
    out = []
    for dt_ in DTYPES:
        for C in R.LN_C[dt_]:
            for rows in R.LN_ROWS:
                out.append((rows, C, dt_, "plain"))
        out.append((R.LN_BIG[0], R.LN_BIG[1], dt_, "plain"))
        out.append((9, R.LN_EMIT_MAX_C, dt_, "plain"))
        for kind in R.LN_KINDS:
            out.append((*R.LN_CLASS_SHAPE[dt_], dt_, kind))
    return out


# ================================================================================================= (1) references
@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
@pytest.mark.parametrize("kind", R.LN_KINDS)
def test_layernorm_reference_is_the_oracle_and_autograd(dtype, kind):
    inp = R.ln_inputs(*R.LN_CLASS_SHAPE[dtype], dtype, kind)
    fw = R.ln_fwd_ref(inp)
    x = inp["x"].double().requires_grad_(True)
    g = inp["gamma"].double().requires_grad_(True)
    b = inp["beta"].double().requires_grad_(True)
    y = O.layer_norm(x, g, b, R.LN_EPS)
    assert close(fw["y"], y.detach())
    y.backward(inp["dy"].double())
    bw = R.ln_bwd_ref(inp, fw["mean"], fw["rstd"], accumulate=True, emit=True)
    assert close(bw["dx"], x.grad + inp["old"].double())
    assert close(bw["dgamma"], g.grad + inp["bases"][0].double()) and close(bw["dbeta"], b.grad + inp["bases"][1].double())
    assert close(bw["colsum"], bw["dx"].sum(0) + inp["bases"][2].double())
    # Dropout behind the LayerNorm: autograd through the masked output
    keep, sc = ln_keep(inp)
    x.grad = None
    (O.layer_norm(x, g, b, R.LN_EPS) * keep * sc).backward(inp["dy"].double())
    bd = R.ln_bwd_ref(inp, fw["mean"], fw["rstd"], accumulate=False, keep_dy=keep, scale_dy=sc)
    assert close(bd["dx"], x.grad)
    fd = R.ln_fwd_ref(inp, keep, sc)
    assert close(fd["y"], y.detach() * keep * sc)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
@pytest.mark.parametrize("V,ld", [(5, 8), (2049, 2056)])
@pytest.mark.parametrize("kind", R.XENT_KINDS)
def test_xent_reference_is_cross_entropy_and_autograd(V, ld, kind, dtype):
    inp = R.xent_inputs(V, ld, dtype, kind)
    ref = R.xent_ref(inp)
    z = inp["logits"][inp["rows"], :V].double().requires_grad_(True)
    tg = torch.tensor(inp["targets"])
    nll = torch.nn.functional.cross_entropy(z, tg, reduction="none")
    (nll.sum() * ref["gs"]).backward()
    assert close(ref["loss"][inp["rows"]], nll.detach())
    assert close(ref["g"][inp["rows"], :V] / ref["gs"], z.grad / ref["gs"])
    assert float(ref["g"][R.xent_zero_mask(inp)].abs().max()) == 0.0


def test_linear_xent_reference_is_the_mixed_log_sum_exp():
    inp = R.xent_inputs(2049, 2056, BF16, "normal")
    x, w, logits, inp2 = R.xent_lm_operands(inp)
    ref = R.xent_ref(inp2, lm=(x, w))
    rows, tg = inp2["rows"], torch.tensor(inp2["targets"])
    z = inp2["logits"][rows, :2049].double()
    zt = (x.double() @ w.double())[rows, tg]
    assert close(z, logits[rows, :2049].double())
    zmix = z.clone()
    zmix[torch.arange(len(rows)), tg] = zt
    assert close(ref["loss"][rows], torch.logsumexp(zmix, -1) - zt, 1e-10)
    assert float((z[torch.arange(len(rows)), tg] - zt).abs().max()) > 0      # the target logit IS off the grid somewhere


@pytest.mark.parametrize("kind", R.SM_KINDS)
def test_softmax_reference_is_torch_softmax_and_autograd(kind):
    s = R.sm_inputs(9, 65, kind)
    ref = R.sm_ref(s, 3)
    x = s.double().requires_grad_(True)
    p = torch.softmax(x, -1)
    assert close(ref["p"], p.detach())
    dp = R.randn((9, 65), 42)
    p.backward(dp)
    assert close(R.sm_bwd_ref(p.detach(), dp)["dp"], x.grad)
    m = R.sm_ref(R.sm_inputs(15, 5, kind), 5, mask_mode=1)
    add = torch.from_numpy((1.0 - O.decoder_mask(5)) * np.float32(-1e9)).repeat(3, 1)
    want = torch.softmax(torch.where(add != 0, R.sm_inputs(15, 5, kind) + add, R.sm_inputs(15, 5, kind)).double(), -1)
    assert close(m["p"], want)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
def test_embedding_reference_is_gather_and_index_add(dtype):
    inp = R.emb_inputs(65, 8, dtype)
    ref = R.emb_ref(inp)
    ids = O.decoder_input_ids(inp["labels"], R.EMB_START).long().reshape(-1)
    assert torch.equal(ids, ref["ids"])
    assert close(ref["out64"], inp["table"].double()[ids] + inp["pe"].double().repeat(inp["B"], 1))
    want = torch.zeros((R.EMB_ROWS, 8), dtype=F64)
    want.index_add_(0, ids, inp["dy"].double())
    assert close(ref["dtable"], want)
    # the forward's stated output is the fp32 sum rounded once
    assert float((ref["out"].double() - ref["out64"]).abs().max()) <= (2.0 ** -8 if dtype == BF16 else U) * float(ref["out64"].abs().max())


# ================================================================================================= (2) feasibility
@pytest.mark.parametrize("rows,C,dtype,kind", ln_all_cases(), ids=lambda v: R.dname(v) if isinstance(v, torch.dtype) else str(v))
def test_layernorm_bounds_admit_fp32(rows, C, dtype, kind):
    inp = R.ln_inputs(rows, C, dtype, kind)
    keep, sc = ln_keep(inp)
    keep2, _ = ln_keep(inp, 1)
    emit = C <= R.LN_EMIT_MAX_C
    for acc in (False, True):
        for kd in (None, keep2):
            fwd, bwd, (m32, r32) = R.ln_fp32(inp, acc, keep_dy=kd, scale_dy=sc, emit=emit, keep=keep if emit else None, scale=sc,
                                             keep_y=kd, scale_y=sc)
            assert R.check_ln_fwd(fwd, R.ln_fwd_ref(inp, kd, sc)) <= 1.0
            ref = R.ln_bwd_ref(inp, m32, r32, acc, keep_dy=kd, scale_dy=sc, emit=emit, keep=keep if emit else None, scale=sc)
            rr = R.ratios_ln_bwd(bwd, ref)
            assert max(rr.values()) <= 1.0, rr


def xent_all_cases():
    return [(V, ld, dt_, k) for dt_, shapes in ((BF16, R.XENT_BF16), (F32, R.XENT_F32)) for V, ld in shapes for k in R.XENT_KINDS]


@pytest.mark.parametrize("V,ld,dtype,kind", xent_all_cases(), ids=lambda v: R.dname(v) if isinstance(v, torch.dtype) else str(v))
def test_xent_bounds_admit_fp32_and_inputs_are_as_named(V, ld, dtype, kind):
    inp = R.xent_inputs(V, ld, dtype, kind)
    ref = R.xent_ref(inp)
    rr = R.ratios_xent(R.xent_fp32(inp), ref)
    assert max(rr.values()) <= 1.0, rr
    # (4) no scored gradient below 2^-100; pads and last-position rows NaN on entry; targets where the names say
    assert float(ref["g"][inp["rows"], :V].abs().min()) >= R.TINY
    assert bool(torch.isnan(inp["logits"].float()[R.xent_zero_mask(inp)]).all())
    assert not bool(torch.isnan(inp["logits"].float()[~R.xent_zero_mask(inp)]).any())
    want = [c for c in (0, 7, 8, V - 1, 2047, 2048, 34815, 34816) if c < V]
    assert set(inp["targets"]) == set(want)
    for r, c in zip(inp["rows"], inp["targets"]):
        assert int(inp["labels"][r // R.XENT_S, r % R.XENT_S + 1]) == c
    if kind == "dom-target":
        assert bool((ref["z"].argmax(-1) == torch.tensor(inp["targets"])).all())
    if kind == "dom-other":
        assert not bool((ref["z"].argmax(-1) == torch.tensor(inp["targets"])).any())
    assert R.xent_kernel_kind(V, ld, dtype) == ("fp32" if dtype == F32 else "generic" if ld > 53248 else "onchip")


def test_xent_targets_sit_on_the_seams():
    t = R.xent_targets(53241)
    assert set(t) == {0, 7, 8, 53240, 2047, 2048, 34815, 34816}
    assert {c >> 3 for c in (7, 8)} == {0, 1}                                   # a chunk edge
    assert {(c >> 3) // 256 for c in (2047, 2048)} == {0, 1}                    # a slot edge
    assert {(c >> 3) // 256 for c in (34815, 34816)} == {R.XREG_SLOTS - 1, R.XREG_SLOTS}   # registers | LDS


@pytest.mark.parametrize("V,ld,kind", [(2049, 2056, "normal"), (2049, 2056, "dom-target"), (53250, 53256, "normal"),
                                       (53250, 53256, "dom-target")])
def test_linear_xent_bound_admits_fp32(V, ld, kind):
    x, w, logits, inp = R.xent_lm_operands(R.xent_inputs(V, ld, BF16, kind))
    ref = R.xent_ref(inp, lm=(x, w))
    rows, tg = inp["rows"], torch.tensor(inp["targets"])
    z = logits[rows, :V].float()
    zt = (x.float() @ w.float())[rows, tg]
    m = z.max(-1).values
    e = torch.exp(z - m[:, None])
    rest = (e.sum(-1) - e[torch.arange(len(rows)), tg]).clamp_min(0)
    loss = torch.zeros(R.XENT_B * R.XENT_S)
    loss[rows] = torch.log1p(rest * torch.exp(m - zt))
    assert R.ratio(loss, ref["loss"], ref["loss_b"]) <= 1.0
    if kind == "normal":   # (a dominant target leaves rest = sum - e_t with the sum's whole absolute error: no 1e-5 there)
        moved = ref["loss"].clone()
        moved[rows[3]] *= 1.0 + 1e-5
        assert R.ratio(moved, ref["loss"], ref["loss_b"]) > 1.0


def sm_cases():
    out = [(3 * R.sm_tq(Tk), R.sm_tq(Tk), Tk, 0, k) for Tk in R.SM_TK for k in R.SM_KINDS]
    out += [(3 * T, T, T, 1, k) for T in R.SM_MASK_T for k in ("normal", "dominant")]
    return out


@pytest.mark.parametrize("rows,Tq,Tk,mask,kind", sm_cases())
def test_softmax_bounds_admit_fp32(rows, Tq, Tk, mask, kind):
    s = R.sm_inputs(rows, Tk, kind)
    ref = R.sm_ref(s, Tq, mask)
    assert R.check_sm_fwd(dict(p=R.sm_fp32(s, Tq, mask)), ref) <= 1.0
    assert rows % 4 != 0
    # (4) masked keys are exactly 0 in the reference, nothing else lies below 2^-100; a fully masked row is uniform
    assert float(ref["p"][ref["masked"]].abs().max() if ref["masked"].any() else 0.0) == 0.0
    assert float(ref["p"][~ref["masked"]].min()) >= R.TINY
    if mask:   # (a dominant score above 32 survives the fp32 addition of -1e9, whose ulp is 64: that row is not uniform)
        assert int(ref["full"].sum()) == 3 and (kind != "normal" or bool((ref["p"][ref["full"]] == 1.0 / Tk).all()))
    p32 = ref["p"].float()
    dp = R.randn((rows, Tk), 42).float()
    got = p32 * (dp - (p32 * dp).sum(-1, keepdim=True))
    assert R.check_sm_bwd(dict(dp=got), R.sm_bwd_ref(p32, dp)) <= 1.0


def test_softmax_bias_form_straddles_two_batches():
    H, Tq, B, Tk = R.SM_BIAS_H, R.SM_BIAS_TQ, R.SM_BIAS_B, 65
    assert (H * Tq) % 4 != 0 and H * Tq > 4          # rows 4..7 of one workgroup belong to batches 0 and 1
    s = R.sm_inputs(B * H * Tq, Tk)
    kb = torch.where(R.randn((B, Tk), 43) > 0.5, -10000.0, 0.0).float()
    ref = R.sm_ref(s, Tq, key_bias=kb, rows_per_batch=H * Tq)
    assert R.check_sm_fwd(dict(p=R.sm_fp32(s, Tq, key_bias=kb, rows_per_batch=H * Tq)), ref) <= 1.0
    rolled = R.sm_ref(s, Tq, key_bias=kb.roll(1, 0), rows_per_batch=H * Tq)     # the neighbouring batch's bias
    assert R.check_sm_fwd(dict(p=rolled["p"]), ref) > 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
@pytest.mark.parametrize("D", R.EMB_D)
@pytest.mark.parametrize("n", list(R.EMB_BS))
def test_embedding_bound_admits_fp32_and_counts_are_present(n, D, dtype):
    inp = R.emb_inputs(n, D, dtype)
    ref = R.emb_ref(inp)
    assert R.check_emb_bwd(dict(dtable=R.emb_bwd_fp32(inp)), ref) <= 1.0
    for i, k in R.EMB_COUNTS.items():
        assert int(ref["count"][i]) == k
    assert int(ref["count"][R.EMB_START]) == inp["B"] + 1            # position 0 of every sequence and one label
    assert int(inp["labels"].min()) >= 0 and int(inp["labels"].max()) < R.EMB_ROWS
    assert int((~ref["touched"]).sum()) > 0


@pytest.mark.parametrize("n", R.SUM_N)
def test_sum_scale_bound_admits_fp32(n):
    x = R.sum_inputs(n)
    ref = R.sum_ref(x)
    assert R.check_sum(dict(out=x.sum() * np.float32(R.SUM_SCALE)), ref) <= 1.0
    if n > 1:
        assert R.check_sum(dict(out=(x[:-1].sum()) * np.float32(R.SUM_SCALE)), ref) > 1.0


# ================================================================================================= (3) tightness
@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
def test_layernorm_mutations_exceed_the_bounds(dtype):
    rows, C = R.LN_CLASS_SHAPE[dtype]
    inp = R.ln_inputs(rows, C, dtype, "plain")
    keep, sc = ln_keep(inp)
    fw = R.ln_fwd_ref(inp)
    bw = R.ln_bwd_ref(inp, fw["mean"], fw["rstd"], True, emit=True, keep=keep, scale=sc)
    good_f = {k: fw[k].clone() for k in ("y", "mean", "rstd")}
    good_b = {k: bw[k].clone() for k in ("dx", "dgamma", "dbeta", "colsum", "masked")}
    assert R.check_ln_fwd(good_f, fw) == 0.0 and R.check_ln_bwd(good_b, bw) == 0.0
    r = 5
    c = int(torch.nonzero(keep[r])[3])

    def f(**kw):
        return R.ratios_ln_fwd({**good_f, **kw}, fw)

    def b(**kw):
        return R.ratios_ln_bwd({**good_b, **kw}, bw)

    m = fw["mean"].clone()
    m[r] += 1e-3 * float(fw["var"][r].sqrt())
    assert f(mean=m)["mean"] > 1.0
    rs = fw["rstd"].clone()
    rs[r] *= 1.0 + 1e-3
    assert f(rstd=rs)["rstd"] > 1.0
    if dtype == F32:
        g1 = dict(inp, gamma=inp["gamma"].clone())
        g1["gamma"][c] = 1.0                                       # gamma taken as 1 in one column
        assert f(y=R.ln_fwd_ref(g1)["y"])["y"] > 1.0
        assert b(dx=R.ln_bwd_ref(g1, fw["mean"], fw["rstd"], True)["dx"])["dx"] > 1.0
        d = bw["dx"].clone()
        d[r] -= inp["old"][r].double()                             # one row's old dx not accumulated
        assert b(dx=d)["dx"] > 1.0
        rr = b(dgamma=bw["dgamma"] - torch.nn.functional.one_hot(torch.tensor(c), C) * (bw["dyeff"] * bw["xhat"])[r, c],
               dbeta=bw["dbeta"] - torch.nn.functional.one_hot(torch.tensor(c), C) * bw["dyeff"][r, c],
               colsum=bw["colsum"] - torch.nn.functional.one_hot(torch.tensor(c), C) * bw["masked"][r, c])
        assert keep[r, c] and min(rr["dgamma"], rr["dbeta"], rr["colsum"]) > 1.0, rr
        dr, dc = [int(v[0]) for v in torch.nonzero(~keep, as_tuple=True)]
        mk = bw["masked"].clone()
        mk[dr, dc] = bw["dx"][dr, dc] * sc                         # an element kept where the host generator drops it
        assert b(masked=mk)["masked"] > 1.0
    y_ref = R.to_dtype(fw["y"], dtype).double()
    dx_ref = R.to_dtype(bw["dx"], dtype).double()
    assert f(y=y_ref)["y"] <= 1.0 and b(dx=dx_ref)["dx"] <= 1.0     # the rounded reference itself passes
    assert f(y=ulp_step(y_ref, (r, c), dtype))["y"] > 1.0
    assert b(dx=ulp_step(dx_ref, (r, c), dtype))["dx"] > 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
def test_xent_mutations_exceed_the_bounds(dtype):
    V, ld = (2049, 2056) if dtype == BF16 else (1021, 1024)
    inp = R.xent_inputs(V, ld, dtype, "normal")
    ref = R.xent_ref(inp)
    good = dict(g=ref["g"].clone(), loss=ref["loss"].clone())
    assert R.check_xent(good, ref) == 0.0
    row, i = inp["rows"][2], 2
    t = inp["targets"][i]
    col = (t + 100) % V

    def gr(g):
        return R.ratios_xent(dict(g=g, loss=good["loss"]), ref)["g"]

    g = good["g"].clone()
    g[row, col] = 0.0
    assert gr(g) > 1.0                                              # a non-target column set to 0
    top = int(ref["p"][i].argmax()) >> 3 << 3
    short = 1.0 - float(ref["p"][i, top:top + 8].sum())            # normalised by a sum that leaves out one 8-column chunk
    g = good["g"].clone()
    g[row, :V] = (ref["p"][i] / short - torch.nn.functional.one_hot(torch.tensor(t), V)) * ref["gs"]
    assert gr(g) > 1.0
    g = good["g"].clone()
    g[row, t] += ref["gs"]
    g[row, t + 1] -= ref["gs"]                                      # the -grad_scale placed at target + 1
    assert gr(g) > 1.0
    g = good["g"].clone()
    g[row, V] = 1e-30                                               # a nonzero pad column
    assert gr(g) > 1.0
    g = good["g"].clone()
    g[R.XENT_S - 1, 3] = 1e-30                                      # a nonzero last-position row
    assert gr(g) > 1.0
    ls = good["loss"].clone()
    ls[row] *= 1.0 + 1e-5
    assert R.ratios_xent(dict(g=good["g"], loss=ls), ref)["loss"] > 1.0
    ls = good["loss"].clone()
    ls[R.XENT_S - 1] = 1e-30
    assert R.ratios_xent(dict(g=good["g"], loss=ls), ref)["loss"] > 1.0


def test_softmax_mutations_exceed_the_bounds():
    s = R.sm_inputs(15, 5)
    ref = R.sm_ref(s, 5, mask_mode=1)
    assert R.check_sm_fwd(dict(p=R.sm_ref(s, 5, mask_mode=1, mask_shift=1)["p"]), ref) > 1.0    # the mask edge one key on
    assert R.check_sm_fwd(dict(p=R.sm_ref(s, 5, mask_mode=1, mask_shift=-1)["p"]), ref) > 1.0
    s = R.sm_inputs(9, 65)                                                                      # key 64: lane 0's second element
    ref = R.sm_ref(s, 3)
    p = ref["p"].clone()
    r = int(p[:, -1].argmax())
    p[r] = p[r] / (1.0 - p[r, -1])                                                            # normalised without the last key
    assert R.check_sm_fwd(dict(p=p), ref) > 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
def test_embedding_mutations_exceed_the_bounds(dtype):
    inp = R.emb_inputs(130, 264, dtype)
    ref = R.emb_ref(inp)
    assert R.check_emb_bwd(dict(dtable=ref["dtable"].clone()), ref) == 0.0
    pos = int(torch.nonzero(ref["ids"] == 5)[-1])
    d = ref["dtable"].clone()
    d[5] -= inp["dy"][pos].double()                               # one of 17 occurrences dropped
    assert R.check_emb_bwd(dict(dtable=d), ref) > 1.0
    d = ref["dtable"].clone()
    assert int(ref["count"][3]) == 8 and int(ref["count"][4]) == 9
    d[4] = ref["dtable"][3]                                        # id 3's row written one row down
    assert R.check_emb_bwd(dict(dtable=d), ref) > 1.0


# ================================================================================================= restated launch rules
def test_layernorm_launch_rules():
    assert [R.ln_nch(c, F32) for c in R.LN_C[F32]] == [1, 1, 2, 3, 4, 8, 8]
    assert [R.ln_nch(c, BF16) for c in R.LN_C[BF16]] == [1, 1, 2, 3, 4, 4]
    for dt_ in DTYPES:   # a last chunk of one lane: C is one vector past a multiple of 64 vectors
        v = R.ln_vec(dt_)
        assert sum(1 for c in R.LN_C[dt_] if (c // v) % 64 == 1) >= 4
    assert R.ln_bwd_blocks(17) == (2, 2) and R.ln_bwd_blocks(9) == (1, 2)      # 17: wave 0 of workgroup 0 takes rows 0 and 16
    assert R.ln_bwd_blocks(4097) == (171, 3) and R.ln_fwd_rows_per_wave(4097) == 2 and R.ln_fwd_rows_per_wave(4096) == 1
    assert 8 * 3 * R.LN_EMIT_MAX_C * 4 <= 160 * 1024 < 8 * 3 * (R.LN_EMIT_MAX_C + 8) * 4
    assert math.isclose(DO.keep_scale(R.LN_DROP_P), 4.0 / 3.0, rel_tol=1e-3)
