"""tmi_ctc_posteriors (csrc/ctc_post.hip) through the C ABI, against the float64 reference and the derived bounds of
tests/_ctc_post_ref.py (checked by tests/test_ctc_post_cpu.py).

Every input and output lies inside a larger buffer of 7.0 / NaN guards (integers: 7 / a large negative) with padded
strides and two spare frames behind every clip, compared bit for bit after the call wherever the contract says nothing is
written: the guard zones, the stride padding, rows past frame_lens[n], columns past V, states past S, tokens past
label_lens[n], and every input.  nll / infeasible must equal tmi_ctc_forward's on the same buffers bit for bit.  Measured
/ bound goes through ``_margins.within`` under the names "ctc post ..." with the bound 1; no bound is fitted to what the
kernels give.  The long shapes are held to the same (there loose) bound and, beside it, to the exact statements about the call's
own bits (``test_long``)."""
import math

import numpy as np
import pytest
import torch

import _ctc_post_ref as P
import _ctc_ref as C
from _margins import within

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
TMI_ERR_INVALID = -1
PAD = 64
BLANK = 0


def _L():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib as L
    return L


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


def i32(dev, x):
    return torch.tensor(np.asarray(x), dtype=I32, device=dev)


def launch(dev, items, V, L_max=None, T_max=None, grad=True, zero_infinity=0):
    """items: (lp float64 [>= T, V], labels, T).  One call of tmi_ctc_posteriors and one of tmi_ctc_forward on the same
    buffers; asserts the guards, the untouched regions and the inputs.  -> dict of the raw outputs (host tensors) with
    ``items``: per item the dict that ``P.ratios`` takes."""
    lib = _L().lib()
    N = len(items)
    L_max = L_max or min(max(max(len(lab) for _, lab, _ in items), 1) + 2, 511)   # (padded, up to the limit)
    T_max = T_max or max(max(T for _, _, T in items), 1) + 2                       # (two spare frames: garbage behind every clip)
    SW = 2 * L_max + 1
    lp_st, lp_sn = V + 3, T_max * (V + 3) + 5
    oc_st, oc_sn = V + 1, T_max * (V + 1) + 3
    gr_st, gr_sn = V + 2, T_max * (V + 2) + 7

    def fill_lp(h):   # (behind frame_lens[n] the guard pattern stays: 7.0 / NaN, never read)
        for n, (lp, _, T) in enumerate(items):
            if T > 0:
                h[n * lp_sn:n * lp_sn + T_max * lp_st].view(T_max, lp_st)[:T, :V] = torch.from_numpy(np.asarray(lp)[:T]).float()

    def fill_lab(h):   # (behind label_lens[n] the guard pattern stays: 7 or a large negative, never read)
        for n, (_, lab, _) in enumerate(items):
            h.view(N, L_max)[n, :len(lab)] = torch.from_numpy(np.asarray(lab, dtype=np.int64)).to(I32)
    LP, LAB = G(dev, F32, N * lp_sn, fill_lp), G(dev, I32, N * L_max, fill_lab)
    LL, FL = G(dev, I32, N, lambda h: h.copy_(torch.tensor([len(lab) for _, lab, _ in items], dtype=I32))), \
        G(dev, I32, N, lambda h: h.copy_(torch.tensor([T for _, _, T in items], dtype=I32)))
    nll, bad, fnll, fbad = G(dev, F32, N), G(dev, I32, N), G(dev, F32, N), G(dev, I32, N)
    gam_, occ, grd = G(dev, F32, N * T_max * SW), G(dev, F32, N * oc_sn), G(dev, F32, N * gr_sn)
    tf, tc = G(dev, F32, N * L_max), G(dev, F32, N * L_max)
    rc = lib.tmi_ctc_posteriors(LP.v.data_ptr(), lp_sn, lp_st, V, LAB.v.data_ptr(), LL.v.data_ptr(), FL.v.data_ptr(), BLANK,
                                nll.v.data_ptr(), bad.v.data_ptr(), gam_.v.data_ptr(), occ.v.data_ptr(), oc_sn, oc_st,
                                grd.v.data_ptr() if grad else None, gr_sn, gr_st, tf.v.data_ptr(), tc.v.data_ptr(), N, L_max,
                                T_max, zero_infinity, stream())
    assert rc == 0, lib.tmi_last_error()
    rc = lib.tmi_ctc_forward(LP.v.data_ptr(), lp_sn, lp_st, LAB.v.data_ptr(), LL.v.data_ptr(), FL.v.data_ptr(), BLANK,
                             fnll.v.data_ptr(), fbad.v.data_ptr(), N, L_max, T_max, zero_infinity, stream())
    assert rc == 0, lib.tmi_last_error()
    torch.cuda.synchronize()
    for b, what in ((LP, "logp"), (LAB, "labels"), (LL, "label_lens"), (FL, "frame_lens")):
        assert b.same_where(), f"the input {what} was written"
    none = torch.zeros(N, dtype=torch.bool)
    assert nll.same_where(none) and bad.same_where(none)
    assert torch.equal(bits(nll.now()), bits(fnll.now())), ("nll is not tmi_ctc_forward's", nll.now(), fnll.now())
    assert torch.equal(bad.now(), fbad.now()), "infeasible is not tmi_ctc_forward's"
    k_g, k_l = torch.ones(N, T_max, SW, dtype=torch.bool), torch.ones(N, L_max, dtype=torch.bool)
    k_o, k_r = torch.ones(N * oc_sn, dtype=torch.bool), torch.ones(N * gr_sn, dtype=torch.bool)
    for n, (_, lab, T) in enumerate(items):
        T, S = max(T, 0), 2 * len(lab) + 1
        k_g[n, :T, :S] = False
        k_l[n, :len(lab)] = False
        k_o[n * oc_sn:n * oc_sn + T_max * oc_st].view(T_max, oc_st)[:T, :V] = False
        if grad:
            k_r[n * gr_sn:n * gr_sn + T_max * gr_st].view(T_max, gr_st)[:T, :V] = False
    assert gam_.same_where(k_g), "gamma: rows past the clip or states past S"
    assert occ.same_where(k_o), "occ: rows past the clip or columns past V"
    assert grd.same_where(k_r), "grad: rows past the clip or columns past V (all of it when grad is NULL)"
    assert tf.same_where(k_l) and tc.same_where(k_l), "tokens past label_lens[n]"
    res = {"nll": nll.now().clone(), "bad": bad.now().clone(), "gamma": gam_.now().clone(), "occ": occ.now().clone(),
           "grad": grd.now().clone(), "tok_frames": tf.now().clone(), "tok_center": tc.now().clone(), "items": []}
    for n, (_, lab, T) in enumerate(items):
        T, S, L = max(T, 0), 2 * len(lab) + 1, len(lab)
        it = {"gamma": res["gamma"].view(N, T_max, SW)[n, :T, :S].double().numpy(),
              "occ": res["occ"][n * oc_sn:n * oc_sn + T_max * oc_st].view(T_max, oc_st)[:T, :V].double().numpy(),
              "tok_frames": res["tok_frames"].view(N, L_max)[n, :L].double().numpy(),
              "tok_center": res["tok_center"].view(N, L_max)[n, :L].double().numpy(),
              "nll": float(res["nll"][n]), "infeasible": int(res["bad"][n])}
        it["grad"] = res["grad"][n * gr_sn:n * gr_sn + T_max * gr_st].view(T_max, gr_st)[:T, :V].double().numpy()
        res["items"].append(it)
    return res


def same_bits(a, b, keys):
    return [k for k in keys if not torch.equal(bits(a[k]), bits(b[k]))]


def check_item(name, got, ref, zero_infinity=0, grad=True):
    """One item against the float64 reference: flags exactly, nll within the forward bound, everything else within the
    derived bounds; -> the ratios."""
    assert got["infeasible"] == ref["infeasible"], name
    if ref["infeasible"]:
        assert got["nll"] == (0.0 if zero_infinity else math.inf), (name, got["nll"])
    else:
        within(f"ctc post {name} nll", C.ratio([got["nll"]], [ref["nll"]], [ref["bound_nll"]]), 1.0)
    if not grad:
        got = dict(got, grad=ref["grad"])   # (NULL: the buffer was checked to be untouched)
    r = P.ratios(got, ref)
    print(f"ctc post {name}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) + " of the bound;  " + P.bound_report(name, ref))
    for k, v in r.items():
        within(f"ctc post {name} {k}", v, 1.0)
    return r


CASES, LONG = P.cases(), P.long_cases()


@pytest.mark.parametrize("c", CASES, ids=lambda c: c[0])
def test_case(dev, c):
    lp, lab, T, ref = P.case_ref(c)
    V = c[4]
    a = launch(dev, [(lp, lab, T)], V, grad=True, zero_infinity=0)
    check_item(c[0], a["items"][0], ref, 0)
    again = launch(dev, [(lp, lab, T)], V, grad=True, zero_infinity=0)
    assert same_bits(a, again, ("nll", "bad", "gamma", "occ", "grad", "tok_frames", "tok_center")) == [], "two calls differ"
    b = launch(dev, [(lp, lab, T)], V, grad=False, zero_infinity=1)      # grad == NULL, and the other clamp of nll
    check_item(c[0] + " without grad", b["items"][0], ref, 1, grad=False)
    assert same_bits(a, b, ("bad", "gamma", "occ", "tok_frames", "tok_center")) == [], "the result depends on grad"
    if not ref["infeasible"]:
        assert torch.equal(bits(a["nll"]), bits(b["nll"]))
    if c[5] == "exact":   # a single path: gamma is 0 or 1 within the bound
        g = a["items"][0]["gamma"]
        assert np.array_equal(np.round(g), np.round(ref["gamma"]))
        within(f"ctc post {c[0]} single path", C.ratio(g, np.round(g), ref["b_gamma"] + 1e-300), 1.0)


@pytest.mark.parametrize("c", LONG, ids=lambda c: c[0])
def test_long(dev, c):
    """The derived bound is loose here (printed next to what is measured), so the weight lies on what is exact at any
    length and is asserted by ``launch`` and below: nll / infeasible are tmi_ctc_forward's bits, the untouched regions,
    the same bits twice and with grad == NULL.  The identities of the device's own numbers are printed."""
    lp, lab, T, ref = P.case_ref(c)
    V = c[4]
    a = launch(dev, [(lp, lab, T)], V, grad=True, zero_infinity=0)
    check_item(c[0], a["items"][0], ref, 0)
    b = launch(dev, [(lp, lab, T)], V, grad=False, zero_infinity=0)
    assert same_bits(a, b, ("nll", "bad", "gamma", "occ", "tok_frames", "tok_center")) == [], "two calls differ, or grad matters"
    got = a["items"][0]
    print(f"ctc post {c[0]}: rows of occ sum to 1 within {np.abs(got['occ'].sum(axis=1) - 1.0).max():.3e}, expected frames add "
          f"up to T within {abs(got['tok_frames'].sum() + got['occ'][:, BLANK].sum() - T):.3e}, smallest tok_frames "
          f"{got['tok_frames'].min():.6f}; gamma off by {np.abs(got['gamma'] - ref['gamma']).max():.3e}, grad by "
          f"{np.abs(got['grad'] - ref['grad']).max():.3e}, tok_center by {np.abs(got['tok_center'] - ref['tok_center']).max():.3e}")


RAGGED = ["T64 L33 alt", "T17 L9 alt", "T7 L0", "T64 L33 equal", "T64 L63 alt", "T9 L4 equal", "T64 L31 neginf", "T1 L1", "T300 L127"]


def test_ragged_batch_equals_items_alone(dev):
    """One launch over items of every kind - among them a clip without frames (frame_lens 0), items without labels
    (label_lens 0), one without a path and one with -inf log-probs - gives each item the bits it gets alone."""
    V = 32
    items = [P.case_ref(next(c for c in CASES + LONG if c[0] == n)) for n in RAGGED]
    triples = [(lp, lab, T) for lp, lab, T, _ in items]
    triples.insert(2, (items[0][0], items[0][1], 0))                         # frame_lens[n] = 0 with labels
    triples.insert(5, (items[1][0], np.zeros(0, dtype=np.int64), 0))         # frame_lens[n] = 0, label_lens[n] = 0
    refs = [r for *_, r in items]
    refs.insert(2, P.post_ref(items[0][0], items[0][1], 0))
    refs.insert(5, P.post_ref(items[1][0], [], 0))
    both = launch(dev, triples, V)
    again = launch(dev, triples, V)
    assert same_bits(both, again, ("nll", "bad", "gamma", "occ", "grad", "tok_frames", "tok_center")) == [], "two calls differ"
    for n, (tr, ref) in enumerate(zip(triples, refs)):
        check_item(f"ragged item {n}", both["items"][n], ref, 0)
        alone = launch(dev, [tr], V)["items"][0]
        for k in P.KEYS + ("nll",):
            assert np.array_equal(np.asarray(alone[k]).view(np.int64), np.asarray(both["items"][n][k]).view(np.int64)), (n, k)
        assert alone["infeasible"] == both["items"][n]["infeasible"]
    assert both["items"][2]["infeasible"] == 1 and (both["items"][2]["tok_center"] == -1).all()
    assert not both["items"][2]["tok_frames"].any()


def test_values_outside_the_contract_stay_inside_the_tensors(dev):
    """Lengths past the tensors are clamped (the guards around every buffer are checked by ``launch``); a label outside
    [0, V) has log-prob -inf: no path, zeros."""
    V, T, L = 32, 9, 4
    lp = C.lp_inputs(T, V, seed=3)
    for bad_label in (-3, V + 40):
        lab = np.array([5, bad_label, 6, 7], dtype=np.int64)
        out = launch(dev, [(lp, lab, T)], V)
        check_item(f"label {bad_label}", out["items"][0], P.post_ref(lp, lab, T), 0)
        assert out["items"][0]["infeasible"] == 1 and not out["items"][0]["gamma"].any()
    # label_lens / frame_lens beyond L_max / T_max, and a negative label length: the kernel clamps, nothing leaves the tensors
    lib = _L().lib()
    lab = C.labels_for("alt", L, V, 1)
    ref = P.post_ref(lp, lab, T)
    for ll_v, fl_v, L_eff, T_eff in ((L + 50, T + 1000, L, T), (-7, T, 0, T)):
        LP = G(dev, F32, T * V, lambda h: h.view(T, V).copy_(torch.from_numpy(lp).float()))
        LAB = G(dev, I32, L, lambda h: h.copy_(torch.from_numpy(lab).to(I32)))
        nll, bad = G(dev, F32, 1), G(dev, I32, 1)
        gm, oc, gr = G(dev, F32, T * (2 * L + 1)), G(dev, F32, T * V), G(dev, F32, T * V)
        tf, tc = G(dev, F32, L), G(dev, F32, L)
        ll, fl = i32(dev, [ll_v]), i32(dev, [fl_v])
        rc = lib.tmi_ctc_posteriors(LP.v.data_ptr(), T * V, V, V, LAB.v.data_ptr(), ll.data_ptr(), fl.data_ptr(), BLANK, nll.v.data_ptr(), bad.v.data_ptr(), gm.v.data_ptr(),
                                    oc.v.data_ptr(), T * V, V, gr.v.data_ptr(), T * V, V, tf.v.data_ptr(), tc.v.data_ptr(), 1, L,
                                    T, 0, stream())
        assert rc == 0, lib.tmi_last_error()
        torch.cuda.synchronize()
        none = torch.zeros(1, dtype=torch.bool)
        k_g, k_l = torch.ones(T, 2 * L + 1, dtype=torch.bool), torch.ones(L, dtype=torch.bool)
        k_g[:T_eff, :2 * L_eff + 1] = False
        k_l[:L_eff] = False
        full = torch.zeros(T * V, dtype=torch.bool)
        assert LP.same_where() and LAB.same_where() and nll.same_where(none) and bad.same_where(none)
        assert gm.same_where(k_g) and oc.same_where(full) and gr.same_where(full) and tf.same_where(k_l) and tc.same_where(k_l)
        if L_eff == L:
            got = {"gamma": gm.now().view(T, -1).double().numpy(), "occ": oc.now().view(T, V).double().numpy(),
                   "grad": gr.now().view(T, V).double().numpy(), "tok_frames": tf.now().double().numpy(),
                   "tok_center": tc.now().double().numpy(), "nll": float(nll.now()[0]), "infeasible": int(bad.now()[0])}
            check_item("clamped lengths", got, ref, 0)


def test_invalid_arguments(dev):
    lib = _L().lib()
    N, T, L, V = 2, 16, 4, 32
    lp = torch.zeros(N, T, V, device=dev)
    lab = torch.ones(N, L, dtype=I32, device=dev)
    ll, fl = i32(dev, [L, L]), i32(dev, [T, T])
    f = {k: G(dev, F32, N * T * V) for k in ("nll", "gamma", "occ", "grad", "tf", "tc")}
    bad = G(dev, I32, N)
    order = ("lp", "sn", "st_", "V", "lab", "ll", "fl", "blank", "nll", "bad", "gamma", "occ", "osn", "ost", "grad", "gsn", "gst",
             "tf", "tc", "N", "L", "T", "zi")
    good = dict(lp=lp.data_ptr(), sn=T * V, st_=V, V=V, lab=lab.data_ptr(), ll=ll.data_ptr(), fl=fl.data_ptr(), blank=0,
                nll=f["nll"].v.data_ptr(), bad=bad.v.data_ptr(), gamma=f["gamma"].v.data_ptr(), occ=f["occ"].v.data_ptr(),
                osn=T * V, ost=V, grad=f["grad"].v.data_ptr(), gsn=T * V, gst=V, tf=f["tf"].v.data_ptr(), tc=f["tc"].v.data_ptr(),
                N=N, L=L, T=T, zi=0)
    bads = [dict(lp=None), dict(lab=None), dict(ll=None), dict(fl=None), dict(nll=None), dict(bad=None), dict(gamma=None),
            dict(occ=None), dict(tf=None), dict(tc=None), dict(N=0), dict(N=65536), dict(L=0), dict(L=512), dict(T=0),
            dict(T=4097, sn=4097 * V, osn=4097 * V, gsn=4097 * V), dict(V=1), dict(V=65, st_=65, ost=65, gst=65, sn=T * 65,
                                                                               osn=T * 65, gsn=T * 65),
            dict(blank=-1), dict(blank=V), dict(st_=V - 1), dict(sn=T * V - 1), dict(ost=V - 1), dict(osn=T * V - 1),
            dict(gst=V - 1), dict(gsn=T * V - 1), dict(zi=2), dict(zi=-1), dict(lp=lp.data_ptr() + 2),
            dict(gamma=f["gamma"].v.data_ptr() + 2), dict(grad=f["grad"].v.data_ptr() + 1), dict(tc=f["tc"].v.data_ptr() + 2)]
    for kw in bads:
        a = dict(good)
        a.update(kw)
        assert lib.tmi_ctc_posteriors(*[a[k] for k in order], stream()) == TMI_ERR_INVALID, kw
        msg = lib.tmi_last_error()
        assert b"tmi_ctc_posteriors" in msg and b"N <= 65535" in msg and b"L_max <= 511" in msg and b"T_max <= 4096" in msg
        assert b"V <= 64" in msg and b"blank < V" in msg and b"lp_sn >= T_max lp_st" in msg
    torch.cuda.synchronize()
    for g in list(f.values()) + [bad]:   # nothing was launched
        assert g.same_where()
    # grad == NULL with strides of 0 is a good call
    a = dict(good, grad=None, gsn=0, gst=0)
    assert lib.tmi_ctc_posteriors(*[a[k] for k in order], stream()) == 0, lib.tmi_last_error()
    torch.cuda.synchronize()
    assert f["grad"].same_where()
