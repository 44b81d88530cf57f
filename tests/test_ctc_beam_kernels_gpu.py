"""tmi_ctc_beam (csrc/ctc_beam.hip) through the C ABI, against the float64 reference and the derived bounds of
tests/_ctc_beam_ref.py (checked by tests/test_ctc_beam_cpu.py).

Exact tier: the decided cases of ``EXACT_CASES`` - tokens, lengths and n_beams EQUAL the reference, every score within its
own bound - batched by (V, K) into ragged launches, and every item bit-equal to the item run alone.  Invariant tier, for
shapes that cannot be decided (K = 16, V = 64, T = 300): descending scores, distinct sequences, tokens in range and not
the blank, lengths <= T, every score <= the sequence's float64 log-likelihood plus ``pruned_score_bound`` (pruning only
loses mass), and the same bits from a second call.

Every input and output lies inside a larger buffer of 7.0 / NaN guards (integers: 7 / a large negative) with a padded
frame stride, compared bit for bit after the call wherever the contract says nothing is written: the guard zones, the
tokens past a length, the inputs, and everything when a call is refused."""
import math

import numpy as np
import pytest
import torch

import _ctc_beam_ref as R
import _ctc_ref as C
from _margins import within

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
TMI_ERR_INVALID = -1
PAD = 64
BLANK = 0
_REF = {}


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


def ref_of(c):
    if c[0] not in _REF:
        lp = R.case_lp(c)
        _REF[c[0]] = (lp, R.beam_ref(lp, c[3]))
    return _REF[c[0]]


def launch(dev, lps, frame_lens, K, V, T_max, blank=BLANK, extra_items=0):
    """One tmi_ctc_beam call over the items ``lps`` (float64 [>= T, V] each) with a frame stride of V + 3; the buffers hold
    ``extra_items`` items more than the call is told of.  -> dict of the guarded buffers and the outputs on the host."""
    lib = _L().lib()
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
    rc = lib.tmi_ctc_beam(b["lp"].v.data_ptr(), T_max * st, st, V, b["fl"].v.data_ptr(), blank, K, b["tok"].v.data_ptr(),
                          b["len"].v.data_ptr(), b["sc"].v.data_ptr(), b["nb"].v.data_ptr(), N, T_max, b["ws"].v.data_ptr(),
                          nbytes, stream())
    assert rc == 0, lib.tmi_last_error()
    torch.cuda.synchronize()
    assert b["lp"].same_where() and b["fl"].same_where(), "an input was written"
    tail = torch.zeros(b["ws"].n, dtype=torch.bool)
    tail[nbytes // 4:] = True
    assert b["ws"].same_where(tail), "the workspace's tail was written"
    out = {"tok": b["tok"].now().view(Nb, K, T_max), "len": b["len"].now().view(Nb, K), "sc": b["sc"].now().view(Nb, K),
           "nb": b["nb"].now()}
    # nothing past a length, past N
    ln = out["len"][:N].clamp(0, T_max)
    keep = torch.ones(Nb, K, T_max, dtype=torch.bool)
    keep[:N] = torch.arange(T_max)[None, None, :] >= ln[:, :, None]
    assert b["tok"].same_where(keep), "tokens were written past a length or past N"
    for name, per in (("len", K), ("sc", K), ("nb", 1)):
        k = torch.zeros(Nb, per, dtype=torch.bool)
        k[N:] = True
        assert b[name].same_where(k), f"{name} was written past N"
    out["bufs"] = b
    return out


def check_item(name, out, n, ref, K):
    nb = int(out["nb"][n])
    assert nb == ref["n_beams"], (name, nb, ref["n_beams"])
    assert out["len"][n, :nb].tolist() == ref["lengths"], name
    assert (out["len"][n, nb:] == 0).all() and torch.isneginf(out["sc"][n, nb:]).all(), (name, "ranks past n_beams")
    for r, seq in enumerate(ref["tokens"]):
        assert tuple(out["tok"][n, r, :len(seq)].tolist()) == seq, (name, r)
    ratio = C.ratio(out["sc"][n, :nb].double().numpy(), ref["scores"], ref["bounds"])
    print(f"ctc beam {name}: scores at {ratio:.4f} of their bounds")
    within("ctc beam exact scores", ratio, 1.0, name)


GROUPS = sorted({(c[2], c[3]) for c in R.EXACT_CASES})


@pytest.mark.parametrize("V,K", GROUPS, ids=lambda v: str(v))
def test_exact_tier_batched_and_alone(dev, V, K):
    cases = [c for c in R.EXACT_CASES if (c[2], c[3]) == (V, K)]
    lps = [ref_of(c)[0] for c in cases]
    T_max = max(c[4] for c in cases)
    out = launch(dev, lps, [c[4] for c in cases], K, V, T_max, extra_items=1)
    for n, c in enumerate(cases):
        check_item(c[0], out, n, ref_of(c)[1], K)
    for n, c in enumerate(cases):     # every item alone, in a tensor of its own length: the same bits
        alone = launch(dev, [lps[n]], [c[4]], K, V, c[4])
        nb = int(out["nb"][n])
        assert int(alone["nb"][0]) == nb and torch.equal(alone["len"][0], out["len"][n]), c[0]
        assert torch.equal(bits(alone["sc"][0]), bits(out["sc"][n])), c[0]
        for r in range(nb):
            ln = int(out["len"][n, r])
            assert torch.equal(alone["tok"][0, r, :ln], out["tok"][n, r, :ln]), (c[0], r)


def test_lengths_outside_the_tensor_and_items_without_frames(dev):
    """frame_lens 0 and negative: the start state.  frame_lens past T_max: clamped.  blank = V - 1."""
    c = next(x for x in R.EXACT_CASES if x[0] == "V32 K4 T100")
    lp, ref = ref_of(c)
    out = launch(dev, [lp, lp, lp, lp], [0, 100, 5000, -3], 4, 32, 100)
    for n in (0, 3):
        assert int(out["nb"][n]) == 1 and out["len"][n].tolist() == [0, 0, 0, 0]
        assert out["sc"][n].tolist() == [0.0, -math.inf, -math.inf, -math.inf]
    for n in (1, 2):
        check_item(f"{c[0]} item {n}", out, n, ref, 4)
    assert torch.equal(bits(out["sc"][1]), bits(out["sc"][2]))
    # another blank: the columns rotated so that the blank is the last one gives the same search with tokens shifted
    rot = np.concatenate([lp[:, 1:], lp[:, :1]], axis=1)
    o2 = launch(dev, [rot], [100], 4, 32, 100, blank=31)
    assert int(o2["nb"][0]) == ref["n_beams"] and o2["len"][0, :ref["n_beams"]].tolist() == ref["lengths"]
    for r, seq in enumerate(ref["tokens"]):
        assert tuple((o2["tok"][0, r, :len(seq)] + 1).tolist()) == seq
    # candidate order is by symbol, which the rotation changes only among equal scores: the scores are the same bits
    assert torch.equal(bits(o2["sc"][0]), bits(out["sc"][1]))


@pytest.mark.parametrize("kind", ["near-uniform", "peaky"])
def test_invariant_tier(dev, kind):
    K, V, T = 16, 64, 300
    lps = [C.lp_inputs(T, V, 11), C.lp_inputs(T, V, 12, scale=0.3)] if kind == "near-uniform" else \
        [R.peaky_lp(T, V, 21), R.peaky_lp(T, V, 22, boost=4.0)]
    fls = [T, T - 37]
    out = launch(dev, lps, fls, K, V, T)
    again = launch(dev, lps, fls, K, V, T)
    for name in ("tok", "len", "sc", "nb"):
        assert torch.equal(bits(out["bufs"][name].t), bits(again["bufs"][name].t)), f"{name}: a second call gave other bits"
    for n, (lp, fl) in enumerate(zip(lps, fls)):
        nb = int(out["nb"][n])
        assert nb == K
        sc = out["sc"][n].double().numpy()
        assert np.isfinite(sc).all() and (np.diff(sc) <= 0).all(), "scores are not descending"
        seqs = [tuple(out["tok"][n, r, :int(out["len"][n, r])].tolist()) for r in range(nb)]
        assert len(set(seqs)) == nb, "two ranks hold the same sequence"
        bound = R.pruned_score_bound(lp, fl)
        worst = -math.inf
        for r, seq in enumerate(seqs):
            assert 0 <= len(seq) <= fl and all(0 <= s < V and s != BLANK for s in seq), (n, r)
            full = -C.ctc_forward_ref(lp, np.array(seq, dtype=np.int64), fl)["nll"]
            worst = max(worst, (sc[r] - full) / bound)
        print(f"ctc beam invariant {kind} item {n}: score - log-likelihood at most {worst:.4f} of the bound {bound:.3e}")
        within("ctc beam pruned score above the log-likelihood", max(worst, 0.0), 1.0, (kind, n))


def test_invalid_arguments_launch_nothing(dev):
    lib = _L().lib()
    N, K, V, T = 2, 4, 32, 16
    st = V
    lp = G(dev, F32, N * T * st, lambda h: h.copy_(torch.from_numpy(np.stack([C.lp_inputs(T, V, 1), C.lp_inputs(T, V, 2)])
                                                                    .astype(np.float32)).reshape(-1)))
    fl = G(dev, I32, N, lambda h: h.fill_(T))
    outs = {"tok": G(dev, I32, N * K * T), "len": G(dev, I32, N * K), "sc": G(dev, F32, N * K), "nb": G(dev, I32, N)}
    nbytes = lib.tmi_ctc_beam_workspace_bytes(N, K, T)
    ws = G(dev, I32, nbytes // 4)
    order = ("lp", "sn", "st", "V", "fl", "blank", "K", "tok", "len", "sc", "nb", "N", "T", "ws", "wsb")
    good = dict(lp=lp.v.data_ptr(), sn=T * st, st=st, V=V, fl=fl.v.data_ptr(), blank=0, K=K, tok=outs["tok"].v.data_ptr(),
                len=outs["len"].v.data_ptr(), sc=outs["sc"].v.data_ptr(), nb=outs["nb"].v.data_ptr(), N=N, T=T,
                ws=ws.v.data_ptr(), wsb=nbytes)
    bads = [dict(lp=None), dict(fl=None), dict(tok=None), dict(len=None), dict(sc=None), dict(nb=None), dict(ws=None),
            dict(lp=good["lp"] + 2), dict(fl=good["fl"] + 1), dict(tok=good["tok"] + 2), dict(len=good["len"] + 2),
            dict(sc=good["sc"] + 2), dict(nb=good["nb"] + 2), dict(ws=good["ws"] + 4),
            dict(N=0), dict(N=65536), dict(K=0), dict(K=17), dict(V=1), dict(V=65, st=65, sn=T * 65), dict(V=V, st=V - 1),
            dict(T=0), dict(T=65537), dict(sn=T * st - 1), dict(blank=-1), dict(blank=V), dict(wsb=nbytes - 1), dict(wsb=0),
            dict(K=8), dict(N=3)]   # (more beams or items than the workspace was sized for)
    for kw in bads:
        a = dict(good)
        a.update(kw)
        assert lib.tmi_ctc_beam(*[a[k] for k in order], stream()) == TMI_ERR_INVALID, kw
        assert b"tmi_ctc_beam" in lib.tmi_last_error()
    torch.cuda.synchronize()
    for name, g in dict(outs, ws=ws, lp=lp, fl=fl).items():
        assert g.same_where(), f"a refused call wrote {name}"
    assert lib.tmi_ctc_beam(*[good[k] for k in order], stream()) == 0, lib.tmi_last_error()
    torch.cuda.synchronize()
    assert int(outs["nb"].now()[0]) == K


def test_ops_wrapper_validates_and_runs(dev):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops
    c = next(x for x in R.EXACT_CASES if x[0] == "V32 K4 T100")
    lp64, ref = ref_of(c)
    N, K, T, V = 2, 4, 100, 32
    lp = torch.from_numpy(np.stack([lp64, lp64]).astype(np.float32)).to(dev)
    fl = torch.tensor([T, T], dtype=I32, device=dev)

    def bufs():
        return (torch.full((N, K, T), -1, dtype=I32, device=dev), torch.zeros(N, K, dtype=I32, device=dev),
                torch.zeros(N, K, dtype=F32, device=dev), torch.zeros(N, dtype=I32, device=dev),
                torch.empty(ops.ctc_beam_workspace_elems(N, K, T), dtype=I32, device=dev))
    tok, ln, sc, nb, ws = bufs()
    ops.ctc_beam(lp, fl, 0, K, tok, ln, sc, nb, ws)
    torch.cuda.synchronize()
    out = {"tok": tok.cpu(), "len": ln.cpu(), "sc": sc.cpu(), "nb": nb.cpu()}
    check_item("ops.ctc_beam", out, 1, ref, K)
    assert (tok.cpu()[1, 0, ref["lengths"][0]:] == -1).all()
    for bad in (dict(K=17), dict(K=0), dict(tok=tok[:, :2]), dict(ws=ws[:-1]), dict(sc=sc.double()), dict(lp=lp.double()),
                dict(ln=ln[:1]), dict(nb=nb.float())):
        a = dict(lp=lp, fl=fl, K=K, tok=tok, ln=ln, sc=sc, nb=nb, ws=ws)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.ctc_beam(a["lp"], a["fl"], 0, a["K"], a["tok"], a["ln"], a["sc"], a["nb"], a["ws"])
    from tethys_speech_amd._lib import TmiError
    with pytest.raises(TmiError):
        ops.ctc_beam(lp, fl, V, K, tok, ln, sc, nb, ws)     # the blank outside the row: refused by the library
