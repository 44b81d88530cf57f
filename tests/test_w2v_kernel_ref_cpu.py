"""The references of tests/_w2v_kernel_ref.py against the oracle and autograd (1e-12 relative), and every property of the
seeded inputs that tests/test_w2v_kernels_gpu.py relies on: runs without a GPU."""
import math

import numpy as np
import pytest
import torch

import _w2v_kernel_ref as R
from oracle import wav2vec2_oracle as V
from oracle import whisper_oracle as O

F64 = torch.float64
TOL = 1e-12


def close(a, b):
    return R.rel_max(a, b) <= TOL


# ------------------------------------------------------------------------------------------- the references themselves
@pytest.mark.parametrize("B,T,C,G,eps", [(2, 7, 16, 4, 1e-5), (1, 13, 24, 1, 1e-3), (3, 5, 32, 8, 1e-5)])
def test_groupnorm_gelu_reference_is_the_oracle_and_its_autograd(B, T, C, G, eps):
    x = R.randn((B, T, C), 1, 1.5) + 0.3
    dy, gamma, beta = R.randn((B, T, C), 2), R.randn((C,), 3, 0.2) + 1.0, R.randn((C,), 4, 0.2)
    r = R.gn_ref(x, dy, gamma, beta, G, eps)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    y = O.gelu_erf(V.group_norm(xr, gr, br, G, eps=eps))
    y.backward(dy)
    assert close(r["y"], y) and close(r["dx"], xr.grad) and close(r["dgamma"], gr.grad) and close(r["dbeta"], br.grad)
    assert close(R.gelu(x), O.gelu_erf(x))
    z = x.clone().requires_grad_(True)
    O.gelu_erf(z).sum().backward()
    assert close(R.gelu_grad(x), z.grad)
    xg = x.reshape(B, T, G, C // G)
    assert close(r["stats"][..., 0], xg.mean(dim=(1, 3)))
    assert close(r["stats"][..., 1], 1.0 / torch.sqrt(xg.var(dim=(1, 3), unbiased=False) + eps))
    # sums: the two means the input gradient is built from, by their definition on autograd's dxhat
    xh = ((xg - xg.mean(dim=(1, 3), keepdim=True)) / torch.sqrt(xg.var(dim=(1, 3), unbiased=False, keepdim=True) + eps)).reshape(B, T, C)
    xh = xh.detach().requires_grad_(True)
    O.gelu_erf(gamma * xh + beta).backward(dy)
    assert close(r["sums"][..., 0], xh.grad.reshape(B, T, G, -1).mean(dim=(1, 3)))
    assert close(r["sums"][..., 1], (xh.grad * xh.detach()).reshape(B, T, G, -1).mean(dim=(1, 3)))


@pytest.mark.parametrize("B,Tin,C,G", [(2, 5, 8, 1), (2, 7, 16, 2), (1, 333, 16, 2), (3, 52, 24, 3)])
def test_fir_reference_is_the_oracle_conv_and_its_autograd(B, Tin, C, G):
    audio, w, gamma, beta, dy = R.fir_inputs((B, Tin, C, G), torch.float32)
    T, pl, pr = R.same_pad(Tin, 10, 5)
    assert (T, pl, pr) == O.same_pad(Tin, 10, 5)
    r = R.fir_ref(audio, w, gamma, beta, dy, G, 1e-5)
    wr, gr, br = (t.double().requires_grad_(True) for t in (w, gamma, beta))
    u = V.conv1d_same(audio.double().unsqueeze(-1), wr, None, 5)
    assert close(u, O.conv1d_same(audio.double().unsqueeze(-1), wr, None, 5)) and close(r["u"], u)
    y = O.gelu_erf(V.group_norm(u, gr, br, G))
    y.backward(dy.double())
    assert close(r["y"], y) and close(r["dW"], wr.grad) and close(r["dgamma"], gr.grad) and close(r["dbeta"], br.grad)


@pytest.mark.parametrize("B,T,C,G,k", [(1, 5, 24, 3, 8), (3, 20, 64, 1, 7), (2, 9, 32, 4, 8)])
def test_pack_maps_make_the_grouped_conv(B, T, C, G, k):
    """pack -> per-group window product with the packed weights -> unpack is the oracle's grouped conv1d_same; the backward
    weight form is the forward one flipped in time and transposed per group."""
    Cg = C // G
    x, w = R.randn((B * T, C), 5), R.randn((k, Cg, C), 6, 0.2)
    _, pl, _ = O.same_pad(T, k, 1)
    Tp = T + k - 1
    xg = R.pack_ref(x, B, T, C, G, Tp, pl)
    wf, wb = R.weight_pack_ref(w, k, Cg, G)
    M = B * Tp - (k - 1)
    win = torch.stack([xg[:, j:j + M, :] for j in range(k)], 2).reshape(G, M, k * Cg)   # row m = rows m .. m + k - 1
    yg = torch.zeros((G, B * Tp, Cg), dtype=F64)
    yg[:, :M] = win @ wf
    out = R.unpack_ref(yg, B, T, C, G, Tp, 0)
    ref = V.conv1d_same(x.reshape(B, T, C), w, None, 1, groups=G)
    assert close(out.reshape(B, T, C), ref)
    assert torch.equal(wb.reshape(G, k, Cg, Cg), wf.reshape(G, k, Cg, Cg).flip(1).transpose(2, 3))
    # unpack undoes pack at the same offset, element for element
    assert torch.equal(R.unpack_ref(R.pack_ref(x, B, T, C, G, Tp + 3, 2), B, T, C, G, Tp + 3, 2), x)


@pytest.mark.parametrize("name,shape", R.CONTRASTIVE_SHAPES[:1] + [("small", (2, 9, 5, False)), ("small-per-time", (2, 9, 5, True))])
def test_contrastive_reference_is_the_oracle_and_its_autograd(name, shape):
    B, T, Nn, per_time = shape
    D = 6
    h, q = R.randn((B, T, D), 7, 0.5).requires_grad_(True), R.randn((B, T, D), 8, 0.5)
    rng = np.random.default_rng(9)
    neg = torch.from_numpy(rng.integers(0, T, size=((T if per_time else B), Nn)).astype(np.int32))
    temp = float(np.float32(0.125))   # exactly representable: the reference's fl32(1 / temperature) is the oracle's 1 / temperature
    _, loss = V.contrastive_loss(h, q, neg[None].expand(B, -1, -1) if per_time else neg, temp)
    loss.backward()
    S = torch.einsum("btd,bsd->bts", h.detach(), q)
    rl, dS, sampled, _ = R.contrastive_ref(S, neg, temp, 0.5, per_time)
    assert abs(float(rl.mean()) - float(loss)) <= TOL * abs(float(loss))
    # dS is d(sum of rows) * 0.5 (exact power of two); the oracle's loss is the mean
    assert close(torch.einsum("bts,bsd->btd", dS, q) / (0.5 * B * T), h.grad)
    assert float(dS[~sampled].abs().max()) == 0.0 if (~sampled).any() else True


def test_quantiser_references():
    h, cb, _ = R.vq_inputs((20, 2, 9, 5), torch.float32)
    d = R.vq_dist(h, cb)
    hh = h.double().reshape(20, 2, 5)
    brute = torch.stack([torch.stack([((hh[:, g] - cb[g, c].double()) ** 2).sum(-1) for c in range(9)], -1) for g in range(2)], 1)
    assert close(d, brute)
    d[3, 1, 7] = d[3, 1, 2] = d[3, 1].min() - 1.0   # a tie: the first index wins
    idx = R.vq_argmin(d)
    assert int(idx[3, 1]) == 2 and torch.equal(d.gather(-1, idx[..., None]).squeeze(-1), d.min(-1).values)
    # perplexity against the oracle's formula written with one_hot (V:653-660)
    enc = torch.nn.functional.one_hot(idx, 9).double().mean(0).clamp(1e-10, 1.0)
    assert abs(R.perplexity_ref(idx, 9) - float(torch.exp(-(enc * torch.log(enc + 1e-10)).sum(-1)).mean())) <= 1e-12
    assert abs(R.perplexity_ref(torch.zeros((20, 2), dtype=torch.int64), 9) - math.exp(-(math.log(1 + 1e-10) + 8 * 1e-10 * math.log(2e-10)))) <= 1e-12
    # the scatter is the gradient of one_hot @ codebook
    cbr = cb.double().requires_grad_(True)
    dq = R.randn((20, 10), 11)
    q = torch.stack([cbr[g][idx[:, g]] for g in range(2)], 1).reshape(20, 10)
    q.backward(dq)
    s, a, n = R.vq_scatter_ref(idx, dq, 9)
    assert close(s, cbr.grad) and float(n.sum()) == 40.0 and bool((a >= s.abs() - 1e-15).all())


def test_segment_references_and_bf16_rounding():
    g = R.seg_inputs(1000)
    offs = [0, 3, 3, 500, 1000]
    ss = R.segment_sumsq_ref(g, offs)
    assert close(ss, torch.tensor([float(g[a:b].double().norm() ** 2) for a, b in zip(offs[:-1], offs[1:])], dtype=F64))
    assert float(ss[1]) == 0.0
    sc = R.clip_scale_f32(ss.float().numpy(), 1.0)
    assert sc[1] == 1.0 and abs(float(sc[3]) - 1.0 / max(math.sqrt(float(ss[3])), 1.0)) <= 4 * R.U
    x = torch.cat([R.randn((4096,), 12).float(), torch.tensor([1.00390625, 1.01171875, -1.00390625])])   # two ties: 1 + 2^-8, 1 + 3 * 2^-8
    assert torch.equal(R.bf16_rne(x).view(torch.int16), x.to(torch.bfloat16).view(torch.int16))
    assert float(R.bf16_rne(x)[-3]) == 1.0 and float(R.bf16_rne(x)[-2]) == 1.015625


# ------------------------------------------------------------------------------ the inputs the GPU tests are built on
def test_groupnorm_shapes_reach_the_paths_their_names_claim():
    geo = {}
    for name, (B, T, C, G), which in R.GN_SHAPES:
        nch = R.gn_chunks(T)
        rpc = -(-T // nch)
        for vec in ([4] if which == "fp32" else [8] if which == "bf16" else [4, 8]):
            cpr = C // vec
            assert 2048 // (8 // (vec // 4)) % C == 0 or (256 * vec) % C == 0
            assert (C // G) % vec == 0
            geo[(name, vec)] = dict(nch=nch, rpc=rpc, last=T - (nch - 1) * rpc, rstep=max(1, 256 // cpr), per=(C // G) // vec,
                                    nsub=1 if G >= 256 else 256 // G)
    assert geo[("two-chunks-ragged", 4)]["nch"] == 2 and geo[("two-chunks-ragged", 4)]["last"] == 32 < geo[("two-chunks-ragged", 4)]["rpc"] == 33
    assert geo[("32-chunks-of-67-last-36", 4)] == dict(nch=32, rpc=67, last=36, rstep=16, per=2, nsub=32)
    for k in (("rstep1-per1-nsub1-bf16", 8), ("rstep1-per1-nsub1-fp32", 4)):
        assert (geo[k]["rstep"], geo[k]["per"], geo[k]["nsub"]) == (1, 1, 1)
    assert geo[("cg8-bf16", 8)]["per"] == 1 and geo[("one-group", 4)]["nsub"] == 256
    assert geo[("one-row", 8)]["rstep"] == 64 and geo[("one-row", 8)]["last"] == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_groupnorm_input_classes_are_what_they_say(dtype):
    B, T, C, G = R.GN_CLASS_SHAPE
    x, _, _, beta = R.gn_inputs(R.GN_CLASS_SHAPE, dtype, "const")
    xg = x.double().reshape(B, T, G, C // G)
    assert bool((xg[:, :, R.GN_CONST_GROUP] == R.GN_CONST_VALUE).all()) and float(xg[:, :, 0].std()) > 1.0
    r = R.gn_ref(x, x, torch.ones(C), beta, G, 1e-5)
    assert bool((r["stats"][:, R.GN_CONST_GROUP, 1] == 1.0 / math.sqrt(1e-5)).all())
    x, _, _, _ = R.gn_inputs(R.GN_CLASS_SHAPE, dtype, "offset")
    xg = x.double().reshape(B, T, G, C // G)
    ratio = xg.mean(dim=(1, 3)) / xg.std(dim=(1, 3), unbiased=False)
    # "mean / std = 16 in every group": within 4 % of it for every (batch row, group), after the rounding to ``dtype``
    assert float((ratio / R.GN_OFFSET_RATIO - 1.0).abs().max()) <= 0.04, ratio


def test_offset_bound_comes_from_the_two_pass_emulation_and_the_raw_moment_form_misses_it():
    """Measured here (fp32 inputs, shape (2, 65, 64, 4), mean / std = 16): two-pass float32 error of y 7.3e-7, of dx 1.0e-6, of
    the mean 1.2e-7 (all relative to max|ref|), of rstd 1.25e-7 (relative per entry); the bounds are four times those: 2.9e-6,
    4.0e-6, 4.9e-7, 5.0e-7.  E[x^2] - mean^2 from fp32 chunk sums - the
    kernel's form until its statistics were centred on a pivot - has an rstd error of 3.8e-5, 76 times that bound."""
    bounds, meas = R.gn_offset_bounds(torch.float32)
    print("two-pass fp32 emulation, float64 error:", meas, "bounds:", bounds)
    assert all(0.0 < meas[k] <= 2e-6 for k in meas), meas   # the emulation is a sane fp32 computation: a few u
    x, dy, gamma, beta = R.gn_inputs(R.GN_CLASS_SHAPE, torch.float32, "offset")
    ref = R.gn_ref(x, dy, gamma, beta, R.GN_CLASS_SHAPE[3], 1e-5)
    raw = R.gn_one_pass_fp32(x, R.GN_CLASS_SHAPE[3], 1e-5)
    raw_rstd = float(((raw[..., 1].double() - ref["stats"][..., 1]) / ref["stats"][..., 1]).abs().max())
    print("raw-moment form, rstd relative error:", raw_rstd)
    assert raw_rstd > bounds["rstd"]


def test_fir_shapes_reach_the_paths_their_names_claim():
    def fir_chunks(T):
        return max(1, min(64, (T + 99) // 100))
    geo = {}
    for name, (B, Tin, C, G) in R.FIR_SHAPES:
        T = R.same_pad(Tin, 10, 5)[0]
        assert 2048 % C == 0 and (C // G) % 8 == 0
        nf, ng = fir_chunks(T), R.gn_chunks(T)
        rf, rg = -(-T // nf), -(-T // ng)
        parts = B * ng
        ry = 8 if parts >= 64 else 1
        geo[name] = dict(T=T, rstep=256 // (C // 8), fir=(nf, rf, T - (nf - 1) * rf), gn=(ng, rg, T - (ng - 1) * rg), parts=parts,
                         slices=sorted({len(range(y, parts, ry)) for y in range(ry)}))
    assert geo["T1-cpr1-rstep256"]["T"] == 1 and geo["T1-cpr1-rstep256"]["rstep"] == 256 and geo["T2-cg8"]["T"] == 2
    assert geo["rstep1"]["rstep"] == 1
    g = geo["T2113-ragged-both-96-parts"]
    assert g["fir"] == (22, 97, 76) and g["gn"] == (32, 67, 36) and g["parts"] == 96 and g["slices"] == [12]
    g = geo["T900-75-parts"]
    assert g["T"] == 900 and g["parts"] == 75 and g["slices"] == [9, 10]
    audio = R.fir_inputs(R.FIR_SHAPES[4][1], torch.float32, "dc")[0].double()
    assert abs(float(audio.mean()) - 0.25) < 1e-3 and abs(float(audio.std()) - 0.01) < 1e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name,shape", R.VQ_SHAPES)
def test_quantiser_inputs_ambiguous_rows_are_capped_and_ties_are_exact(name, shape, dtype):
    rows, G, Nc, gd = shape
    h, cb, _ = R.vq_inputs(shape, dtype)
    d = R.vq_dist(h, cb)
    ok, decisive = R.vq_judge(R.vq_argmin(d), d, gd)
    assert bool(ok.all())
    amb = float((~decisive).double().mean())
    print(f"{name} {dtype}: ambiguous (row, group) pairs {amb:.4f}")
    assert float((~decisive).any(dim=1).double().mean()) <= 0.01   # at most 1 % of the rows
    # the tie inputs: the copies of code c are exact ties in float64 and the nearest codes of the planted rows
    h, cb, tie_rows = R.vq_inputs(shape, dtype, ties=True)
    d = R.vq_dist(h, cb)
    c = R.VQ_TIE_CODE
    copies = [c + 1] + ([c + 64] if Nc > c + 64 else [])
    assert (name == "rowsG-201-Nc17-gd24") == (len(copies) == 1)
    for r in tie_rows:
        for g in range(G):
            assert all(float(d[r, g, k]) == float(d[r, g, c]) for k in copies)
            assert float(d[r, g, c]) == float(d[r, g].min()) and int(R.vq_argmin(d)[r, g]) == c
            others = torch.cat([d[r, g, :c], d[r, g, c + 2:c + 64], d[r, g, c + 65:]])
            assert float(others.min()) - float(d[r, g, c]) > 4 * float(R.vq_dist_bound(others.min(), gd))   # nothing else is near
    # every other undecided row of the tie inputs is a tie of the same kind: its best code is c, and c's copies aside nothing
    # is within the fp32 bounds of it - so the kernel must answer c there too (vq_tie_rows)
    _, decisive = R.vq_judge(R.vq_argmin(d), d, gd)
    on_c = R.vq_tie_rows(d, gd)
    assert bool(on_c[tie_rows].all()) and bool((decisive | on_c).all())


def test_vq_bwd_shape_wraps_its_grid():
    rows, G, Nc, gd = R.VQ_BWD_SHAPE
    assert -(-rows * G * gd // 256) == 2200 > 2048
    idx = R.perplexity_patterns(rows, G, Nc)["spread"]
    n = R.vq_scatter_ref(idx, torch.zeros((rows, G * gd)), Nc)[2]
    assert 60 <= float(n.min()) and float(n.max()) <= 80   # "about 70 rows per code"


@pytest.mark.parametrize("name,shape", R.CONTRASTIVE_SHAPES)
def test_contrastive_inputs_have_repeats_hits_and_large_logits(name, shape):
    B, T, Nn, per_time = shape
    S, neg = R.contrastive_inputs(shape)
    assert neg.shape == ((T if per_time else B), Nn) and (Nn == 0 or (0 <= int(neg.min()) and int(neg.max()) < T))
    if Nn >= 100:
        rows = neg.numpy()
        assert all(len(set(r.tolist())) < Nn for r in rows)   # repeats in every index row
        hits = [(t in rows[t if per_time else b]) for b in range(B) for t in range(T)]
        assert any(hits) and not all(hits)                     # some rows sample their own t, some do not
        _, _, sampled, _ = R.contrastive_ref(S, neg, R.CONTRASTIVE_TEMP, R.CONTRASTIVE_GRAD_SCALE, per_time)
        assert bool((~sampled).any())                          # unsampled columns exist: their dS must be exactly 0
    if T == 1:
        assert int(neg.abs().max()) == 0
    big, _ = R.contrastive_inputs(shape, "large")
    if T > 1:
        assert 1500.0 <= float(big.abs().max()) / R.CONTRASTIVE_TEMP <= 2001.0
        assert math.isinf(float(torch.exp(torch.tensor(float(big.max()) / R.CONTRASTIVE_TEMP, dtype=torch.float32))))
    dom, _ = R.contrastive_inputs(shape, "dominant")
    rl, _, _, _ = R.contrastive_ref(dom, neg, R.CONTRASTIVE_TEMP, 1.0, per_time)
    if name == "T300-Nn200":   # the positive dominates: the loss is log(1 + number of negatives that are t itself), 0 without such a hit
        hit = torch.tensor([int((neg[b] == t).sum()) for b in range(B) for t in range(T)], dtype=F64)
        assert float((rl - torch.log1p(hit)).abs().max()) < 1e-12 and float(rl[hit == 0].max()) < 1e-100 and float(hit.max()) >= 1 and float(hit.min()) == 0


def test_segment_inputs_straddle_the_clip_threshold():
    g = R.seg_inputs()
    offs = R.SEG_OFFSETS
    ss = R.segment_sumsq_ref(g, offs)
    norms = ss.sqrt().tolist()
    print("segment norms:", norms)
    assert [a % 4 for a in offs[:-1]] == [0, 1, 1, 3, 1] and offs[1] == offs[2]
    # "below the threshold": by more than any fp32 sum error, so the kernel's scale is exactly 1 there; the others are well above
    assert norms[0] < 0.9 * R.SEG_CLIP and norms[1] == 0.0 and norms[2] < 0.9 * R.SEG_CLIP
    assert norms[3] > 1.1 * R.SEG_CLIP and norms[4] > 1.1 * R.SEG_CLIP
    big = R.seg_inputs(R.SEG_BIG_N, 502)
    assert float((big.double() ** 2).sum().sqrt()) > 1.1 * R.SEG_CLIP
    per = (-(-R.SEG_BIG_N // 512) + 3) // 4 * 4
    assert per == 3324 and per // 4 == 831 > 768   # thread i < 831 - 768 = 63 runs one four-in-flight round
