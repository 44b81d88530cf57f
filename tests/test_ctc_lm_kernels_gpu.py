"""tmi_ctc_beam_lm (csrc/ctc_beam.hip) through the C ABI, against the float64 reference and the derived bounds of
tests/_ctc_lm_ref.py (checked by tests/test_ctc_lm_cpu.py).

Exact tier: the decided cases of ``LM_CASES`` - tokens, lengths and n_beams EQUAL the reference; scores, ctc_scores and
lm_scores each within their own bound - batched by (V, K, order) into ragged launches, every item bit-equal to the item
run alone.  Zero weights: the tokens, lengths and scores of tmi_ctc_beam in the same test.  Invariant tier (K = 16, V = 64,
T = 300, order 2, undecidable): descending scores, distinct sequences, scores = ctc_scores + lm_scores in one rounding,
lm_scores the fp32 recomputation along the returned tokens bit for bit, ctc_scores <= the float64 log-likelihood plus
``pruned_score_bound``, the same bits from a second call.

Every input (the table included) and output lies inside a larger buffer of guards with a padded frame stride, as in
tests/test_ctc_beam_kernels_gpu.py, compared bit for bit after the call wherever the contract says nothing is written."""
import math

import numpy as np
import pytest
import torch

import _ctc_beam_ref as R
import _ctc_lm_ref as L
import _ctc_ref as C
from _margins import within

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
TMI_ERR_INVALID = -1
PAD = 64


def _lib():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib as M
    return M.lib()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class G:
    """``n`` payload elements inside guards; ``v`` is the payload on the device, ``host`` the payload as it was sent."""

    def __init__(self, dev, dtype, n, fill=None):
        host = C.guard_pattern(n + 2 * PAD, dtype)
        self.host = host[PAD:PAD + n]
        if fill is not None:
            fill(self.host)
        self.host0, self.t, self.n = host.clone(), host.to(dev), n
        self.v = self.t[PAD:PAD + n]

    def now(self):
        return self.t.cpu()[PAD:PAD + self.n]

    def same_where(self, keep=None):
        """The guard zones and every payload element with ``keep`` set (None: all) are bit for bit what they were."""
        full = torch.ones(self.n + 2 * PAD, dtype=torch.bool)
        if keep is not None:
            full[PAD:PAD + self.n] = torch.as_tensor(keep).reshape(-1)
        return torch.equal(bits(self.t)[full], bits(self.host0)[full])


def stream():
    return torch.cuda.current_stream().cuda_stream


def launch(dev, lps, frame_lens, K, V, T_max, lm=None, order=1, alpha=L.ALPHA, beta=L.BETA, blank=0, extra_items=0):
    """One tmi_ctc_beam_lm call (``lm`` None: tmi_ctc_beam) over the items ``lps`` (float64 [>= T, V] each) with a frame
    stride of V + 3; the buffers hold ``extra_items`` items more than the call is told of.  -> dict of the guarded buffers
    and the outputs on the host."""
    lib = _lib()
    N, st = len(lps), V + 3
    Nb = N + extra_items

    def fill(h):
        v = h.view(Nb, T_max, st)
        for n, lp in enumerate(lps):
            t = min(lp.shape[0], T_max)
            v[n, :t, :V] = torch.from_numpy(np.asarray(lp[:t], dtype=np.float32))
    b = {"lp": G(dev, F32, Nb * T_max * st, fill),
         "fl": G(dev, I32, Nb, lambda h: h[:N].copy_(torch.tensor(frame_lens, dtype=I32))),
         "tok": G(dev, I32, Nb * K * T_max), "len": G(dev, I32, Nb * K), "sc": G(dev, F32, Nb * K), "nb": G(dev, I32, Nb)}
    nbytes = lib.tmi_ctc_beam_workspace_bytes(N, K, T_max)
    assert nbytes == N * K * T_max * 8
    b["ws"] = G(dev, I32, nbytes // 4 + 32)
    if lm is None:
        rc = lib.tmi_ctc_beam(b["lp"].v.data_ptr(), T_max * st, st, V, b["fl"].v.data_ptr(), blank, K, b["tok"].v.data_ptr(),
                              b["len"].v.data_ptr(), b["sc"].v.data_ptr(), b["nb"].v.data_ptr(), N, T_max,
                              b["ws"].v.data_ptr(), nbytes, stream())
        per_rank = ("len", "sc")
    else:
        table = torch.from_numpy(np.asarray(lm, dtype=np.float32).reshape(-1))
        assert table.numel() == V ** order
        b["lm"] = G(dev, F32, V ** order, lambda h: h.copy_(table))
        b["ctc"], b["lms"] = G(dev, F32, Nb * K), G(dev, F32, Nb * K)
        rc = lib.tmi_ctc_beam_lm(b["lp"].v.data_ptr(), T_max * st, st, V, b["fl"].v.data_ptr(), blank, K, b["lm"].v.data_ptr(),
                                 order, alpha, beta, b["tok"].v.data_ptr(), b["len"].v.data_ptr(), b["sc"].v.data_ptr(),
                                 b["ctc"].v.data_ptr(), b["lms"].v.data_ptr(), b["nb"].v.data_ptr(), N, T_max,
                                 b["ws"].v.data_ptr(), nbytes, stream())
        per_rank = ("len", "sc", "ctc", "lms")
    assert rc == 0, lib.tmi_last_error()
    torch.cuda.synchronize()
    assert b["lp"].same_where() and b["fl"].same_where(), "an input was written"
    assert lm is None or b["lm"].same_where(), "the table was written"
    tail = torch.zeros(b["ws"].n, dtype=torch.bool)
    tail[nbytes // 4:] = True
    assert b["ws"].same_where(tail), "the workspace's tail was written"
    out = {"tok": b["tok"].now().view(Nb, K, T_max), "nb": b["nb"].now()}
    for name in per_rank:
        out[name] = b[name].now().view(Nb, K)
    ln = out["len"][:N].clamp(0, T_max)         # nothing past a length, past N
    keep = torch.ones(Nb, K, T_max, dtype=torch.bool)
    keep[:N] = torch.arange(T_max)[None, None, :] >= ln[:, :, None]
    assert b["tok"].same_where(keep), "tokens were written past a length or past N"
    for name, per in [(x, K) for x in per_rank] + [("nb", 1)]:
        k = torch.zeros(Nb, per, dtype=torch.bool)
        k[N:] = True
        assert b[name].same_where(k), f"{name} was written past N"
    out["bufs"] = b
    return out


def check_item(name, out, n, ref):
    nb = int(out["nb"][n])
    assert nb == ref["n_beams"], (name, nb, ref["n_beams"])
    assert out["len"][n, :nb].tolist() == ref["lengths"], name
    assert (out["len"][n, nb:] == 0).all() and torch.isneginf(out["sc"][n, nb:]).all(), (name, "ranks past n_beams")
    assert torch.isneginf(out["ctc"][n, nb:]).all() and (out["lms"][n, nb:] == 0).all(), (name, "ranks past n_beams")
    for r, seq in enumerate(ref["tokens"]):
        assert tuple(out["tok"][n, r, :len(seq)].tolist()) == seq, (name, r)
    if not nb:
        return
    rs = [C.ratio(out[o][n, :nb].double().numpy(), ref[s], ref[b])
          for o, s, b in (("sc", "scores", "bounds"), ("ctc", "ctc_scores", "ctc_bounds"), ("lms", "lm_scores", "lm_bounds"))]
    print(f"ctc lm {name}: scores / ctc_scores / lm_scores at {rs[0]:.4f} / {rs[1]:.4f} / {rs[2]:.4f} of their bounds")
    for what, r in zip(("scores", "ctc_scores", "lm_scores"), rs):
        within(f"ctc lm exact {what}", r, 1.0, name)


def group_key(c):
    return (c[1][2], c[1][3], c[2], c[3], c[4], c[5])      # V, K, order and what fixes the table: seed, -inf share, blank


GROUPS = sorted({group_key(c) for c in L.LM_CASES})


@pytest.mark.parametrize("key", GROUPS, ids=lambda k: "V%d-K%d-o%d-s%d-%g-b%d" % k)
def test_exact_tier_batched_and_alone(dev, key):
    V, K, order, seed, neginf, blank = key
    cases = [c for c in L.LM_CASES if group_key(c) == key]
    inputs = [L.case_ref(c)[0] for c in cases]
    lm = inputs[0][1]
    assert all(np.array_equal(i[1], lm) for i in inputs)
    lps, Ts = [i[0] for i in inputs], [i[3] for i in inputs]
    out = launch(dev, lps, Ts, K, V, max(Ts), lm, order, blank=blank, extra_items=1)
    for n, c in enumerate(cases):
        check_item(c[0], out, n, L.case_ref(c)[1])
    for n, c in enumerate(cases):     # every item alone, in a tensor of its own length: the same bits
        alone = launch(dev, [lps[n]], [Ts[n]], K, V, Ts[n], lm, order, blank=blank)
        nb = int(out["nb"][n])
        assert int(alone["nb"][0]) == nb and torch.equal(alone["len"][0], out["len"][n]), c[0]
        for name in ("sc", "ctc", "lms"):
            assert torch.equal(bits(alone[name][0]), bits(out[name][n])), (c[0], name)
        for r in range(nb):
            ln = int(out["len"][n, r])
            assert torch.equal(alone["tok"][0, r, :ln], out["tok"][n, r, :ln]), (c[0], r)


@pytest.mark.parametrize("V,K", [(3, 16), (3, 3), (32, 4), (4, 8), (64, 16)], ids=str)
def test_zero_weights_give_the_unfused_search(dev, V, K):
    cases = [c for c in R.EXACT_CASES if (c[2], c[3]) == (V, K)]
    lps, Ts = [R.case_lp(c) for c in cases], [c[4] for c in cases]
    plain = launch(dev, lps, Ts, K, V, max(Ts))
    for order in (1, 2):
        fused = launch(dev, lps, Ts, K, V, max(Ts), L.lm_table(V, order, 9), order, alpha=0.0, beta=0.0)
        N = len(cases)
        assert torch.equal(fused["nb"][:N], plain["nb"][:N]) and torch.equal(fused["len"][:N], plain["len"][:N])
        inside = torch.arange(max(Ts))[None, None, :] < plain["len"][:N, :, None]
        assert torch.equal(fused["tok"][:N][inside], plain["tok"][:N][inside])
        assert bool((fused["sc"][:N] == plain["sc"][:N]).all()) and bool((fused["ctc"][:N] == plain["sc"][:N]).all())
        assert bool((fused["lms"][:N] == 0).all())


def test_lengths_outside_the_tensor_and_items_without_frames(dev):
    c = next(x for x in L.LM_CASES if x[0] == "V32 K4 T100 o2")
    (lp, lm, K, T, V, order, blank), ref = L.case_ref(c)
    out = launch(dev, [lp, lp, lp, lp], [0, 100, 5000, -3], K, V, T, lm, order)
    for n in (0, 3):       # the start state: one empty beam, every score 0
        assert int(out["nb"][n]) == 1 and out["len"][n].tolist() == [0, 0, 0, 0]
        assert out["sc"][n].tolist() == [0.0, -math.inf, -math.inf, -math.inf] == out["ctc"][n].tolist()
        assert out["lms"][n].tolist() == [0.0, 0.0, 0.0, 0.0]
    for n in (1, 2):
        check_item(f"{c[0]} item {n}", out, n, ref)
    assert torch.equal(bits(out["sc"][1]), bits(out["sc"][2]))


def test_invariant_tier(dev):
    K, V, T, order = 16, 64, 300, 2
    lps = [R.peaky_lp(T, V, 21), C.lp_inputs(T, V, 12, scale=0.3)]
    fls = [T, T - 37]
    lm = L.lm_table(V, order, 31, neginf=0.05)
    out = launch(dev, lps, fls, K, V, T, lm, order)
    again = launch(dev, lps, fls, K, V, T, lm, order)
    for name in ("tok", "len", "sc", "ctc", "lms", "nb"):
        assert torch.equal(bits(out["bufs"][name].t), bits(again["bufs"][name].t)), f"{name}: a second call gave other bits"
    for n, (lp, fl) in enumerate(zip(lps, fls)):
        nb = int(out["nb"][n])
        assert nb == K
        sc, ctc, lms = (out[x][n].numpy() for x in ("sc", "ctc", "lms"))
        assert np.isfinite(sc).all() and (np.diff(sc) <= 0).all(), "scores are not descending"
        assert (sc == (ctc + lms)).all() and sc.dtype == np.float32, "scores are not ctc_scores + lm_scores in one fp32 add"
        seqs = [tuple(out["tok"][n, r, :int(out["len"][n, r])].tolist()) for r in range(nb)]
        assert len(set(seqs)) == nb, "two ranks hold the same sequence"
        bound = R.pruned_score_bound(lp, fl)
        worst = -math.inf
        for r, seq in enumerate(seqs):
            assert 0 <= len(seq) <= fl and all(0 <= s < V and s != 0 for s in seq), (n, r)
            assert not any(np.isneginf(lm[a, b]) for a, b in zip((0,) + seq, seq)), "a forbidden transition"   # (blank 0 first)
            g = L.g_along(seq, lm, order, L.ALPHA, L.BETA, V)
            assert g.dtype == np.float32 and g.view(np.int32) == lms[r].view(np.int32), (n, r, float(g), float(lms[r]))
            full = -C.ctc_forward_ref(lp, np.array(seq, dtype=np.int64), fl)["nll"]
            worst = max(worst, (float(ctc[r]) - full) / bound)
        print(f"ctc lm invariant item {n}: ctc_score - log-likelihood at most {worst:.4f} of the bound {bound:.3e}")
        within("ctc lm pruned ctc_score above the log-likelihood", max(worst, 0.0), 1.0, n)


def test_invalid_arguments_launch_nothing(dev):
    lib = _lib()
    N, K, V, T, order = 2, 4, 32, 16, 2
    st = V
    lp = G(dev, F32, N * T * st, lambda h: h.copy_(torch.from_numpy(np.stack([C.lp_inputs(T, V, 1), C.lp_inputs(T, V, 2)])
                                                                    .astype(np.float32)).reshape(-1)))
    fl = G(dev, I32, N, lambda h: h.fill_(T))
    lm = G(dev, F32, V ** order, lambda h: h.copy_(torch.from_numpy(L.lm_table(V, order, 3).astype(np.float32).reshape(-1))))
    outs = {"tok": G(dev, I32, N * K * T), "len": G(dev, I32, N * K), "sc": G(dev, F32, N * K), "ctc": G(dev, F32, N * K),
            "lms": G(dev, F32, N * K), "nb": G(dev, I32, N)}
    nbytes = lib.tmi_ctc_beam_workspace_bytes(N, K, T)
    ws = G(dev, I32, nbytes // 4)
    names = ("lp", "sn", "st", "V", "fl", "blank", "K", "lm", "order", "alpha", "beta", "tok", "len", "sc", "ctc", "lms", "nb",
             "N", "T", "ws", "wsb")
    good = dict(lp=lp.v.data_ptr(), sn=T * st, st=st, V=V, fl=fl.v.data_ptr(), blank=0, K=K, lm=lm.v.data_ptr(), order=order,
                alpha=0.5, beta=0.25, tok=outs["tok"].v.data_ptr(), len=outs["len"].v.data_ptr(), sc=outs["sc"].v.data_ptr(),
                ctc=outs["ctc"].v.data_ptr(), lms=outs["lms"].v.data_ptr(), nb=outs["nb"].v.data_ptr(), N=N, T=T,
                ws=ws.v.data_ptr(), wsb=nbytes)
    bads = [dict(lm=None), dict(ctc=None), dict(lms=None), dict(lm=good["lm"] + 2), dict(ctc=good["ctc"] + 2),
            dict(lms=good["lms"] + 1), dict(order=0), dict(order=5), dict(order=-1),
            dict(V=64, st=64, sn=T * 64, order=5),
            dict(alpha=-0.5), dict(alpha=-1e-30), dict(alpha=math.inf), dict(alpha=math.nan), dict(beta=math.inf),
            dict(beta=-math.inf), dict(beta=math.nan),
            # what tmi_ctc_beam refuses
            dict(lp=None), dict(fl=None), dict(tok=None), dict(len=None), dict(sc=None), dict(nb=None), dict(ws=None),
            dict(sc=good["sc"] + 2), dict(ws=good["ws"] + 4), dict(N=0), dict(K=0), dict(K=17), dict(V=1), dict(V=65, st=65, sn=T * 65),
            dict(st=V - 1), dict(T=0), dict(T=65537), dict(sn=T * st - 1), dict(blank=-1), dict(blank=V), dict(wsb=nbytes - 1),
            dict(K=8), dict(N=3)]
    # (V^order > 2^24 cannot be reached inside the other limits - 64^4 is exactly 2^24 - so it is refused with order 5 above)
    for kw in bads:
        a = dict(good)
        a.update(kw)
        assert lib.tmi_ctc_beam_lm(*[a[k] for k in names], stream()) == TMI_ERR_INVALID, kw
        assert b"tmi_ctc_beam_lm" in lib.tmi_last_error()
    torch.cuda.synchronize()
    for name, g in dict(outs, ws=ws, lp=lp, fl=fl, lm=lm).items():
        assert g.same_where(), f"a refused call wrote {name}"
    assert lib.tmi_ctc_beam_lm(*[good[k] for k in names], stream()) == 0, lib.tmi_last_error()
    torch.cuda.synchronize()
    assert int(outs["nb"].now()[0]) == K and lm.same_where() and lp.same_where()


def test_ops_wrapper_validates_and_runs(dev):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops
    c = next(x for x in L.LM_CASES if x[0] == "V32 K4 T100 o3")
    (lp64, lm64, K, T, V, order, blank), ref = L.case_ref(c)
    N = 2
    lp = torch.from_numpy(np.stack([lp64, lp64]).astype(np.float32)).to(dev)
    lm = torch.from_numpy(lm64.astype(np.float32).reshape(-1)).to(dev)
    fl = torch.tensor([T, T], dtype=I32, device=dev)
    tok = torch.full((N, K, T), -1, dtype=I32, device=dev)
    ln, nb = torch.zeros(N, K, dtype=I32, device=dev), torch.zeros(N, dtype=I32, device=dev)
    sc, ctc, lms = (torch.zeros(N, K, dtype=F32, device=dev) for _ in range(3))
    ws = torch.empty(ops.ctc_beam_workspace_elems(N, K, T), dtype=I32, device=dev)
    ops.ctc_beam_lm(lp, fl, 0, K, lm, order, L.ALPHA, L.BETA, tok, ln, sc, ctc, lms, nb, ws)
    torch.cuda.synchronize()
    out = {"tok": tok.cpu(), "len": ln.cpu(), "sc": sc.cpu(), "ctc": ctc.cpu(), "lms": lms.cpu(), "nb": nb.cpu()}
    check_item("ops.ctc_beam_lm", out, 1, ref)
    assert (tok.cpu()[1, 0, ref["lengths"][0]:] == -1).all()
    for bad in (dict(order=0), dict(order=5), dict(order=2), dict(lm=lm[:-1]), dict(lm=lm.double()), dict(lm=lm.cpu()),
                dict(ctc=ctc[:1]), dict(lms=lms.double()), dict(K=17), dict(ws=ws[:-1])):
        a = dict(K=K, lm=lm, order=order, sc=sc, ctc=ctc, lms=lms, ws=ws)
        a.update(bad)
        if bad == dict(order=2):
            a["lm"] = lm[:V * V - 1]
        with pytest.raises(ValueError):
            ops.ctc_beam_lm(lp, fl, 0, a["K"], a["lm"], a["order"], L.ALPHA, L.BETA, tok, ln, a["sc"], a["ctc"], a["lms"], nb, a["ws"])
    from tethys_speech_amd._lib import TmiError
    with pytest.raises(TmiError):
        ops.ctc_beam_lm(lp, fl, 0, K, lm, order, -1.0, 0.0, tok, ln, sc, ctc, lms, nb, ws)     # refused by the library
