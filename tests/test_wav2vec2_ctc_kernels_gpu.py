"""tmi_ctc_logsoftmax, tmi_ctc_greedy, tmi_ctc_forward and tmi_ctc_viterbi (csrc/ctc.hip) through the C ABI, against the
float64 references and the derived bounds of tests/_ctc_ref.py (checked by tests/test_ctc_cpu.py).

Every input and output lies inside a larger buffer of 7.0 / NaN guards (integers: 7 / a large negative) with padded
strides, compared bit for bit after the call wherever the contract says nothing is written: the guard zones, the stride
padding, the columns past V, the entries past out_len[n], label_lens[n] and frame_lens[n], and every input.  Measured /
bound goes through ``_margins.within`` under the names "ctc ..." with the bound 1; no bound is fitted to what the kernels
give.  Integer outputs must EQUAL the reference.

Viterbi, exact cases: log-probs on the grid k / 64, |k| <= 1024, so every fp32 sum is exact and the states, the token
bounds and the total must equal the reference, ties included.  Random cases: a valid path whose float64 score is within
e(P) + e(P*) of the optimum's (the device maximises the fp32 running sums, and rounding is monotone)."""
import math

import numpy as np
import pytest
import torch

import _ctc_ref as C
from _margins import within

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
TMI_ERR_INVALID = -1
PAD = 64
V = C.V_DEFAULT
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


# ============================================================================================== tmi_ctc_logsoftmax
@pytest.mark.parametrize("Vn", [2, 31, 32, 33, 64])
def test_logsoftmax(dev, Vn):
    lib = _L().lib()
    for R in (1, 3, 257):
        ld, lp_ld = Vn + 3, Vn + 5
        x = C.logits_inputs(R, Vn, seed=Vn * 7 + R)
        if R >= 3:
            x[0, :] = 1.25                      # equal logits: argmax 0
            x[1, Vn - 1] = 3.0e4                # one +big value
            x[2, 0:Vn:3] = -np.inf              # -inf entries (never all of them)
            x[2, 1] = 0.5
        if R > 100:
            x[100, :] = x[100, ::-1].max()      # another tie row
            x[101, Vn // 2] = x[101, Vn - 1] = 9.0   # two equal maxima: the smaller column
        logp, amax, bound = C.logsoftmax_ref(x)

        def fill(h):
            h.view(R, ld)[:, :Vn] = torch.from_numpy(x).float()
        X, Y, A = G(dev, F32, R * ld, fill), G(dev, F32, R * lp_ld), G(dev, I32, R)
        rc = lib.tmi_ctc_logsoftmax(X.v.data_ptr(), ld, R, Vn, Y.v.data_ptr(), lp_ld, A.v.data_ptr(), stream())
        assert rc == 0, lib.tmi_last_error()
        torch.cuda.synchronize()
        assert X.same_where(), "the logits were written"
        keep = torch.ones(R, lp_ld, dtype=torch.bool)
        keep[:, :Vn] = False
        assert Y.same_where(keep), "columns past V"
        assert A.same_where(torch.zeros(R, dtype=torch.bool))
        got = Y.now().view(R, lp_ld)[:, :Vn].double().numpy()
        assert np.array_equal(A.now().numpy(), amax), (Vn, R)
        r = C.ratio(got, logp, bound)
        print(f"ctc logsoftmax V{Vn} R{R}: {r:.3f} of its bound")
        within(f"ctc logsoftmax V{Vn}", r, 1.0)


# =================================================================================================== tmi_ctc_greedy
def greedy_items(T):
    """Five items of T frames: runs across every chunk seam; all blank; no blank; a short clip with non-blank garbage
    behind it; no frame at all."""
    g = np.random.default_rng(T)
    a = np.repeat(g.integers(0, V, size=T), g.integers(1, 5, size=T))[:T]
    a[g.random(T) < 0.3] = BLANK
    for seam in (64, 128, 192, 256, 512):   # the wave seams and the chunk seams
        if seam + 4 <= T:
            a[seam - 3:seam + 4] = 5 + seam % 7
    if T > 260:
        a[255], a[256] = 3, 4                 # two tokens that meet at the chunk seam
    noblank = g.integers(1, V, size=T)
    short = max(1, T - 5)
    garbage = np.concatenate([a[:short], np.full(T - short, 9)])
    return [(a, T), (np.full(T, BLANK), T), (noblank, T), (garbage, short), (noblank, 0)]


@pytest.mark.parametrize("T", [1, 63, 64, 65, 255, 256, 257, 700])
def test_greedy(dev, T):
    lib = _L().lib()
    items = greedy_items(T)
    N, lp_ld = len(items), V + 3
    lp = [C.lp_inputs(T, V, seed=T + 31 * n) for n in range(N)]

    def fill_lp(h):
        for n in range(N):
            h.view(N, T, lp_ld)[n, :, :V] = torch.from_numpy(lp[n]).float()

    def fill_a(h):
        for n, (a, _) in enumerate(items):
            h.view(N, T)[n] = torch.from_numpy(a).to(I32)
    A, LP = G(dev, I32, N * T, fill_a), G(dev, F32, N * T * lp_ld, fill_lp)
    fl = i32(dev, [ln for _, ln in items])
    tok, st, en = G(dev, I32, N * T), G(dev, I32, N * T), G(dev, I32, N * T)
    ol, best = G(dev, I32, N), G(dev, F32, N)
    rc = lib.tmi_ctc_greedy(A.v.data_ptr(), LP.v.data_ptr(), lp_ld, fl.data_ptr(), BLANK, tok.v.data_ptr(), ol.v.data_ptr(),
                            st.v.data_ptr(), en.v.data_ptr(), best.v.data_ptr(), N, T, stream())
    assert rc == 0, lib.tmi_last_error()
    torch.cuda.synchronize()
    assert A.same_where() and LP.same_where(), "an input was written"
    keep = torch.ones(N, T, dtype=torch.bool)
    keep_n = torch.zeros(N, dtype=torch.bool)
    worst = 0.0
    for n, (a, ln) in enumerate(items):
        if ln < 1:
            keep_n[n] = True   # skipped entirely: out_len and best_logprob too
            continue
        ref = C.greedy_ref(a, lp[n], ln, BLANK)
        k = len(ref["tokens"])
        assert int(ol.now()[n]) == k, (T, n)
        for buf, name in ((tok, "tokens"), (st, "start"), (en, "end")):
            assert np.array_equal(buf.now().view(N, T)[n, :k].numpy(), ref[name]), (T, n, name)
        keep[n, :k] = False
        worst = max(worst, C.ratio([float(best.now()[n])], [ref["best"]], [ref["best_bound"]]))
    for buf in (tok, st, en):
        assert buf.same_where(keep), "entries at or past out_len[n]"
    assert ol.same_where(keep_n) and best.same_where(keep_n)
    assert int(ol.now()[1]) == 0 and int(ol.now()[2]) == int((np.diff(items[2][0]) != 0).sum()) + 1
    print(f"ctc greedy T{T}: best_logprob at {worst:.3f} of its bound")
    within(f"ctc greedy best_logprob T{T}", worst, 1.0)


# ========================================================================================== tmi_ctc_forward / viterbi
def launch(dev, items, L_max=None, T_max=None, viterbi=False, zero_infinity=0, want_states=True):
    """items: (lp float64 [>= T, V], labels, T).  -> the raw outputs; asserts the guards."""
    lib = _L().lib()
    N = len(items)
    L_max = L_max or min(max(max(len(lab) for _, lab, _ in items), 1) + 2, 511)   # (padded, up to the limit)
    T_max = T_max or max(T for _, _, T in items)
    lp_st, lp_sn = V + 3, T_max * (V + 3) + 5

    def fill_lp(h):
        for n, (lp, _, T) in enumerate(items):
            h[n * lp_sn:n * lp_sn + T_max * lp_st].view(T_max, lp_st)[:T, :V] = torch.from_numpy(np.asarray(lp)[:T]).float()

    def fill_lab(h):   # (behind label_lens[n] the guard pattern stays: 7 or a large negative, never read)
        for n, (_, lab, _) in enumerate(items):
            h.view(N, L_max)[n, :len(lab)] = torch.from_numpy(np.asarray(lab, dtype=np.int64)).to(I32)
    LP, LAB = G(dev, F32, N * lp_sn, fill_lp), G(dev, I32, N * L_max, fill_lab)
    ll, fl = i32(dev, [len(lab) for _, lab, _ in items]), i32(dev, [T for _, _, T in items])
    out, bad = G(dev, F32, N), G(dev, I32, N)
    res = {}
    if not viterbi:
        rc = lib.tmi_ctc_forward(LP.v.data_ptr(), lp_sn, lp_st, LAB.v.data_ptr(), ll.data_ptr(), fl.data_ptr(), BLANK,
                                 out.v.data_ptr(), bad.v.data_ptr(), N, L_max, T_max, zero_infinity, stream())
    else:
        st, en, states = G(dev, I32, N * L_max), G(dev, I32, N * L_max), G(dev, I32, N * T_max)
        nbytes = lib.tmi_ctc_workspace_bytes(N, L_max, T_max)
        assert nbytes > 0
        ws = G(dev, I32, nbytes // 4)
        rc = lib.tmi_ctc_viterbi(LP.v.data_ptr(), lp_sn, lp_st, LAB.v.data_ptr(), ll.data_ptr(), fl.data_ptr(), BLANK,
                                 st.v.data_ptr(), en.v.data_ptr(), out.v.data_ptr(), states.v.data_ptr() if want_states else None,
                                 bad.v.data_ptr(), N, L_max, T_max, ws.v.data_ptr(), nbytes, stream())
    assert rc == 0, lib.tmi_last_error()
    torch.cuda.synchronize()
    assert LP.same_where() and LAB.same_where(), "an input was written"
    none = torch.zeros(N, dtype=torch.bool)
    assert out.same_where(none) and bad.same_where(none)
    res["out"], res["bad"] = out.now().clone(), bad.now().clone()
    if viterbi:
        assert ws.same_where(torch.zeros(ws.n, dtype=torch.bool)), "workspace guards"
        keep_l, keep_t = torch.ones(N, L_max, dtype=torch.bool), torch.ones(N, T_max, dtype=torch.bool)
        for n, (_, lab, T) in enumerate(items):
            keep_l[n, :len(lab)] = False
            keep_t[n, :max(T, 0)] = not want_states
        assert st.same_where(keep_l) and en.same_where(keep_l), "token bounds past label_lens[n]"
        assert states.same_where(keep_t), "states past frame_lens[n]"
        res.update(start=st.now().view(N, L_max).clone(), end=en.now().view(N, L_max).clone(),
                   states=states.now().view(N, T_max).clone())
    return res


CASES = C.forward_cases()
_REF = {}


def fcase(c):
    if c[0] not in _REF:
        lp, lab, T = C.case_inputs(c)
        _REF[c[0]] = (lp, lab, T, C.ctc_forward_ref(lp, lab, T))
    return _REF[c[0]]


def check_forward(name, got, flag, ref, zero_infinity):
    if ref["infeasible"]:
        assert flag == 1 and got == (0.0 if zero_infinity else math.inf), (name, got, flag)
        within(f"ctc forward {name}", 0.0, 1.0)
        return
    assert flag == 0
    r = C.ratio([got], [ref["nll"]], [ref["bound"]])
    print(f"ctc forward {name}: nll {got!r} vs {ref['nll']!r}: {r:.4f} of the bound {ref['bound']:.3e}")
    within(f"ctc forward {name}", r, 1.0)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c[0])
def test_forward(dev, c):
    lp, lab, T, ref = fcase(c)
    a = launch(dev, [(lp, lab, T)], zero_infinity=0)
    b = launch(dev, [(lp, lab, T)], zero_infinity=1)
    check_forward(c[0], float(a["out"][0]), int(a["bad"][0]), ref, 0)
    check_forward(c[0], float(b["out"][0]), int(b["bad"][0]), ref, 1)
    if not ref["infeasible"]:
        assert torch.equal(bits(a["out"]), bits(b["out"]))


RAGGED = ["T300 L33 alt", "T65 L31", "T1 L0", "T38 L20 equal short", "T300 L128"]


def test_forward_ragged_batch_equals_items_alone(dev):
    items = [fcase(next(c for c in CASES if c[0] == n)) for n in RAGGED]
    both = launch(dev, [(lp, lab, T) for lp, lab, T, _ in items])
    again = launch(dev, [(lp, lab, T) for lp, lab, T, _ in items])
    assert torch.equal(bits(both["out"]), bits(again["out"])), "two calls differ"
    for n, (lp, lab, T, ref) in enumerate(items):
        alone = launch(dev, [(lp, lab, T)])
        assert torch.equal(bits(alone["out"]), bits(both["out"][n:n + 1])) and int(alone["bad"][0]) == int(both["bad"][n]), RAGGED[n]
        check_forward(RAGGED[n] + " in a batch", float(both["out"][n]), int(both["bad"][n]), ref, 0)


def test_forward_item_without_frames(dev):
    lp, lab, T, _ = fcase(CASES[0])
    out = launch(dev, [(lp, lab, 0), (lp, lab, T)], T_max=T)
    assert float(out["out"][0]) == math.inf and int(out["bad"][0]) == 1 and int(out["bad"][1]) == 0


# ---------------------------------------------------------------------------------------------------------- Viterbi
def check_viterbi_exact(out, n, lp, lab, T):
    ref = C.viterbi_ref(lp, lab, T)
    L = len(lab)
    assert int(out["bad"][n]) == ref["infeasible"]
    assert float(out["out"][n]) == ref["total"], (T, L, float(out["out"][n]), ref["total"])
    assert np.array_equal(out["start"][n, :L].numpy(), ref["start"]) and np.array_equal(out["end"][n, :L].numpy(), ref["end"]), (T, L)
    if "states" in out and T > 0:
        assert np.array_equal(out["states"][n, :T].numpy(), ref["states"]), (T, L)


# T at the word (16) and walk-back piece (128) edges, S at the wave seams (L 31 / 32, 127 / 128), the largest S
EXACT = [(1, 0, "random"), (1, 1, "random"), (1, 2, "distinct"), (2, 1, "random"), (5, 2, "equal"), (16, 3, "random"),
         (17, 3, "random"), (40, 7, "random"), (65, 20, "equal"), (70, 31, "alt"), (70, 32, "random"), (70, 33, "alt"),
         (128, 40, "random"), (129, 40, "random"), (300, 127, "random"), (300, 128, "distinct"), (38, 20, "equal"),
         (600, 511, "random")]


@pytest.mark.parametrize("shape", EXACT, ids=lambda s: f"T{s[0]}-L{s[1]}-{s[2]}")
def test_viterbi_exact(dev, shape):
    T, L, kind = shape
    lab = C.labels_for(kind, L, V, seed=T + L)
    fine, coarse = C.grid_lp(T, V, seed=T * 3 + L), np.round(C.grid_lp(T, V, seed=T * 5 + L) / 8)   # coarse: most comparisons tie
    out = launch(dev, [(fine, lab, T), (coarse, lab, T), (np.zeros((T, V)), lab, T)], viterbi=True)
    for n, lp in enumerate((fine, coarse, np.zeros((T, V)))):
        check_viterbi_exact(out, n, lp, lab, T)


def test_viterbi_exact_ragged_in_one_launch(dev):
    shapes = [(300, 128, "distinct"), (1, 0, "random"), (38, 20, "equal"), (129, 40, "random"), (70, 33, "alt")]
    items = [(C.grid_lp(T, V, seed=T + 1), C.labels_for(kind, L, V, seed=L), T) for T, L, kind in shapes]
    out = launch(dev, items, viterbi=True)
    again = launch(dev, items, viterbi=True)
    for k in ("out", "bad", "start", "end", "states"):
        assert torch.equal(bits(out[k]), bits(again[k])), k
    for n, (lp, lab, T) in enumerate(items):
        check_viterbi_exact(out, n, lp, lab, T)
    assert int(out["bad"][2]) == 1 and float(out["out"][2]) == -math.inf and bool((out["start"][2, :20] == -1).all())
    assert bool((out["states"][2, :38] == -1).all())
    nostates = launch(dev, items, viterbi=True, want_states=False)   # states == NULL
    for k in ("out", "bad", "start", "end"):
        assert torch.equal(bits(out[k]), bits(nostates[k])), k


@pytest.mark.parametrize("shape", [(65, 31), (300, 128), (700, 200)], ids=lambda s: f"T{s[0]}-L{s[1]}")
def test_viterbi_random(dev, shape):
    T, L = shape
    lp, lab = C.lp_inputs(T, V, seed=T + L), C.labels_for("random", L, V, seed=L)
    out = launch(dev, [(lp, lab, T)], viterbi=True)
    states = out["states"][0, :T].numpy()
    assert C.path_problems(states, lab, T, out["start"][0, :L].numpy(), out["end"][0, :L].numpy()) == []
    ref = C.viterbi_ref(lp, lab, T)
    score = C.path_score(lp, lab, states)
    e_got, e_ref = C.path_bound(lp, lab, states), C.path_bound(lp, lab, ref["states"])
    deficit = ref["total"] - score
    assert deficit >= -1e-9 * abs(ref["total"])
    print(f"ctc viterbi random T{T} L{L}: deficit {deficit:.3e} of {e_got + e_ref:.3e}, total off by "
          f"{abs(float(out['out'][0]) - score):.3e} of {e_got:.3e}")
    within(f"ctc viterbi random T{T} L{L} deficit", max(deficit, 0.0) / (e_got + e_ref), 1.0)
    within(f"ctc viterbi random T{T} L{L} total", abs(float(out["out"][0]) - score) / e_got, 1.0)
    r32 = C.viterbi_ref(lp, lab, T, dtype=np.float32)   # the same fp32 adds: the same answer bit for bit
    assert np.array_equal(states, r32["states"]) and float(out["out"][0]) == r32["total"]


# --------------------------------------------------------------------------------------------------------- refusals
def test_invalid_arguments(dev):
    lib = _L().lib()
    N, T, L, ld = 2, 16, 4, V
    x = torch.zeros(N * T, ld, device=dev)
    lp = torch.zeros(N, T, ld, device=dev)
    am, lab = torch.zeros(N * T, dtype=I32, device=dev), torch.ones(N, L, dtype=I32, device=dev)
    ll, fl = i32(dev, [L, L]), i32(dev, [T, T])
    outs = {k: G(dev, I32, N * T) for k in ("tok", "st", "en", "ol", "bad", "states")}
    f = {k: G(dev, F32, N * T * ld) for k in ("y", "best", "nll")}
    nbytes = lib.tmi_ctc_workspace_bytes(N, L, T)
    ws = torch.zeros(nbytes // 4, dtype=I32, device=dev)
    assert nbytes == N * 1 * (2 * L + 1) * 4
    for bad in ((0, L, T), (65536, L, T), (N, 0, T), (N, 512, T), (N, L, 0), (N, L, 4097)):
        assert lib.tmi_ctc_workspace_bytes(*bad) == -1, bad

    def refused(fn, name, order, good, bads):
        for kw in bads:
            a = dict(good)
            a.update(kw)
            assert fn(*[a[k] for k in order], stream()) == TMI_ERR_INVALID, (name, kw)
            assert name.encode() in lib.tmi_last_error()

    refused(lib.tmi_ctc_logsoftmax, "tmi_ctc_logsoftmax", ("x", "ld", "R", "V", "y", "lp_ld", "am"),
            dict(x=x.data_ptr(), ld=ld, R=N * T, V=V, y=f["y"].v.data_ptr(), lp_ld=ld, am=am.data_ptr()),
            [dict(x=None), dict(y=None), dict(am=None), dict(R=0), dict(V=1), dict(V=65, ld=65, lp_ld=65), dict(ld=V - 1),
             dict(lp_ld=V - 1), dict(x=x.data_ptr() + 2)])
    refused(lib.tmi_ctc_greedy, "tmi_ctc_greedy", ("am", "lp", "lp_ld", "fl", "blank", "tok", "ol", "st", "en", "best", "N", "T"),
            dict(am=am.data_ptr(), lp=lp.data_ptr(), lp_ld=ld, fl=fl.data_ptr(), blank=0, tok=outs["tok"].v.data_ptr(),
                 ol=outs["ol"].v.data_ptr(), st=outs["st"].v.data_ptr(), en=outs["en"].v.data_ptr(), best=f["best"].v.data_ptr(),
                 N=N, T=T),
            [dict(am=None), dict(lp=None), dict(fl=None), dict(tok=None), dict(ol=None), dict(st=None), dict(en=None),
             dict(best=None), dict(N=0), dict(N=65536), dict(T=0), dict(lp_ld=0), dict(blank=-1), dict(lp=lp.data_ptr() + 1)])
    common = dict(lp=lp.data_ptr(), sn=T * ld, st_=ld, lab=lab.data_ptr(), ll=ll.data_ptr(), fl=fl.data_ptr(), blank=0, N=N, L=L,
                  T=T)
    bad_common = [dict(lp=None), dict(lab=None), dict(ll=None), dict(fl=None), dict(N=0), dict(N=65536), dict(L=0), dict(L=512),
                  dict(T=0), dict(st_=0), dict(sn=T * ld - 1), dict(blank=-1), dict(blank=ld), dict(lp=lp.data_ptr() + 2)]
    refused(lib.tmi_ctc_forward, "tmi_ctc_forward", ("lp", "sn", "st_", "lab", "ll", "fl", "blank", "nll", "bad", "N", "L", "T", "zi"),
            dict(common, nll=f["nll"].v.data_ptr(), bad=outs["bad"].v.data_ptr(), zi=0),
            bad_common + [dict(nll=None), dict(bad=None), dict(zi=2), dict(zi=-1), dict(T=2 ** 31 - 16, sn=2 ** 40)])
    refused(lib.tmi_ctc_viterbi, "tmi_ctc_viterbi",
            ("lp", "sn", "st_", "lab", "ll", "fl", "blank", "ts", "te", "tot", "states", "bad", "N", "L", "T", "ws", "nbytes"),
            dict(common, ts=outs["st"].v.data_ptr(), te=outs["en"].v.data_ptr(), tot=f["nll"].v.data_ptr(),
                 states=outs["states"].v.data_ptr(), bad=outs["bad"].v.data_ptr(), ws=ws.data_ptr(), nbytes=nbytes),
            bad_common + [dict(ts=None), dict(te=None), dict(tot=None), dict(bad=None), dict(ws=None), dict(nbytes=nbytes - 1),
                          dict(T=4097, sn=4097 * ld, nbytes=1 << 30), dict(states=outs["states"].v.data_ptr() + 2)])
    torch.cuda.synchronize()
    for g in list(outs.values()) + list(f.values()):   # nothing was launched
        assert g.same_where()
