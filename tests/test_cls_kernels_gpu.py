"""tmi_cls_head_fwd / tmi_cls_head_bwd (csrc/cls_head.hip) through the C ABI, against the float64 reference and the derived
bounds of tests/_cls_ref.py (checked by tests/test_cls_cpu.py).

Every input and output lies inside a larger buffer of 7.0 / NaN guards (integers: 7 / a large negative) with padded
strides, compared bit for bit after the calls wherever the contract says nothing is written: the guard zones, the stride
padding and every input.  Measured / bound goes through ``_margins.within`` under the names "cls ..." with the bound 1; no
bound is fitted to what the kernels give.  ``pred`` and ``label_rank`` are compared with the float64 reference where it
decides them beyond the logit bound (``_cls_ref.decided``); the seeds were picked on the CPU so that at most 1 % of a
case's rows are left out, and the test asserts that cap."""
import numpy as np
import pytest
import torch

import _cls_ref as R
from _margins import within

pytestmark = pytest.mark.gpu

F32, I32, I64 = torch.float32, torch.int32, torch.int64
TMI_ERR_INVALID = -1
PAD = 64
TR = 8   # rows per workgroup of the forward (CH_TR)


def _L():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib as L
    return L


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int64)


def guard_pattern(n, dtype):
    t = torch.full((n,), 7, dtype=dtype)
    t[1::2] = float("nan") if dtype.is_floating_point else -(2 ** 30)
    return t


class G:
    """``n`` payload elements inside guards; ``v`` is the payload on the device, ``host`` the payload as it was sent."""

    def __init__(self, dev, dtype, n, fill=None):
        host = guard_pattern(n + 2 * PAD, dtype)
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


def rows_into(h, a, ld):
    a = torch.as_tensor(np.ascontiguousarray(a))
    h[:a.shape[0] * ld].view(a.shape[0], ld)[:, :a.shape[1]] = a


def flat_into(h, a):
    h.copy_(torch.as_tensor(np.ascontiguousarray(a)).reshape(-1))


def rows_from(g, rows, ld, cols):
    return g.now()[:rows * ld].view(rows, ld)[:, :cols].numpy().copy()


def unwritten(rows, ld, cols):
    k = torch.ones(rows, ld, dtype=torch.bool)
    k[:, :cols] = False
    return k


class Call:
    """One forward call (and optionally one backward call) on guarded buffers with padded strides."""

    def __init__(self, dev, d, N, p=0.0, seed=0, row_index=None, confusion=False, optional=True, labels=True):
        self.dev, self.d, self.N, self.p, self.seed = dev, d, N, float(p), int(seed)
        x = d["x"]
        self.n_src, self.H = x.shape
        self.P, self.C = d["Wc"].shape
        H, P, C = self.H, self.P, self.C
        self.ld_x, self.ld_lg, self.ld_z, self.ld_lp, self.ld_cf = H + 4, C + 3, P + 2, C + 1, C + 5
        self.X = G(dev, F32, self.n_src * self.ld_x, lambda h: rows_into(h, x, self.ld_x))
        self.Wp, self.bp = G(dev, F32, H * P, lambda h: flat_into(h, d["Wp"])), G(dev, F32, P, lambda h: flat_into(h, d["bp"]))
        self.Wc, self.bc = G(dev, F32, P * C, lambda h: flat_into(h, d["Wc"])), G(dev, F32, C, lambda h: flat_into(h, d["bc"]))
        self.idx = None if row_index is None else G(dev, I32, N, lambda h: flat_into(h, np.asarray(row_index, dtype=np.int32)))
        self.row_index = None if row_index is None else np.asarray(row_index)
        self.lab = G(dev, I32, N, lambda h: flat_into(h, d["labels"].astype(np.int32))) if labels else None
        self.logits, self.pred = G(dev, F32, N * self.ld_lg), G(dev, I32, N)
        self.z = G(dev, F32, N * self.ld_z) if optional else None
        self.lp = G(dev, F32, N * self.ld_lp) if optional else None
        self.nll = G(dev, F32, N) if optional else None
        self.rank = G(dev, I32, N) if optional else None
        self.conf = G(dev, I64, C * self.ld_cf, lambda h: h.zero_()) if confusion else None
        self.inputs = [b for b in (self.X, self.Wp, self.bp, self.Wc, self.bc, self.idx, self.lab) if b is not None]

    def gathered(self):
        x = self.d["x"]
        return x[:self.N] if self.row_index is None else x[self.row_index]

    @staticmethod
    def _p(g):
        return None if g is None else g.v.data_ptr()

    def fwd_args(self):
        return [self.X.v.data_ptr(), self.ld_x, self.n_src, self._p(self.idx), self.Wp.v.data_ptr(), self.bp.v.data_ptr(),
                self.Wc.v.data_ptr(), self.bc.v.data_ptr(), self._p(self.lab), self.p, self.seed, self.logits.v.data_ptr(),
                self.ld_lg, self.pred.v.data_ptr(), self._p(self.z), self.ld_z, self._p(self.lp), self.ld_lp, self._p(self.nll),
                self._p(self.rank), self._p(self.conf), self.ld_cf, self.N, self.H, self.P, self.C, stream()]

    def fwd(self, check_table=True):
        lib = _L().lib()
        rc = lib.tmi_cls_head_fwd(*self.fwd_args())
        assert rc == 0, lib.tmi_last_error()
        torch.cuda.synchronize()
        N, P, C = self.N, self.P, self.C
        for b in self.inputs:
            assert b.same_where(), "an input was written"
        none = torch.zeros(N, dtype=torch.bool)
        assert self.logits.same_where(unwritten(N, self.ld_lg, C)) and self.pred.same_where(none)
        out = {"logits": rows_from(self.logits, N, self.ld_lg, C), "pred": self.pred.now().numpy().copy()}
        if self.z is not None:
            assert self.z.same_where(unwritten(N, self.ld_z, P)) and self.lp.same_where(unwritten(N, self.ld_lp, C))
            assert self.nll.same_where(none) and self.rank.same_where(none)
            out.update(z=rows_from(self.z, N, self.ld_z, P), log_probs=rows_from(self.lp, N, self.ld_lp, C),
                       nll=self.nll.now().numpy().copy(), label_rank=self.rank.now().numpy().copy())
        if self.conf is not None:
            assert self.conf.same_where(unwritten(C, self.ld_cf, C))
            out["confusion"] = self.conf.now()[:C * self.ld_cf].view(C, self.ld_cf)[:, :C].numpy().copy()
        self.out = out
        return out

    def bwd_buffers(self):
        lib = _L().lib()
        H, P, C, N = self.H, self.P, self.C, self.N
        nb = lib.tmi_cls_head_workspace_bytes(N, H, P, C)
        chunks = -(-N // 256)
        assert nb == 256 + 4 * (N * P + (chunks * max(H * P + P, P * C + C) if chunks > 1 else 0))
        dev = self.dev
        self.gWp, self.gbp, self.gWc, self.gbc = G(dev, F32, H * P), G(dev, F32, P), G(dev, F32, P * C), G(dev, F32, C)
        self.loss, self.ws = G(dev, F32, 1), G(dev, F32, nb // 4)

    def bwd_args(self):
        return [self.X.v.data_ptr(), self.ld_x, self.n_src, self._p(self.idx), self.Wc.v.data_ptr(), self.lab.v.data_ptr(), self.p,
                self.seed, self.z.v.data_ptr(), self.ld_z, self.lp.v.data_ptr(), self.ld_lp, self.gWp.v.data_ptr(),
                self.gbp.v.data_ptr(), self.gWc.v.data_ptr(), self.gbc.v.data_ptr(), self.loss.v.data_ptr(), self.ws.v.data_ptr(),
                self.ws.n * 4, self.N, self.H, self.P, self.C, stream()]

    def bwd(self):
        lib = _L().lib()
        self.bwd_buffers()
        z0, lp0 = self.z.t.cpu(), self.lp.t.cpu()
        rc = lib.tmi_cls_head_bwd(*self.bwd_args())
        assert rc == 0, lib.tmi_last_error()
        torch.cuda.synchronize()
        for b in self.inputs:
            assert b.same_where(), "an input was written"
        assert torch.equal(bits(self.z.t), bits(z0)) and torch.equal(bits(self.lp.t), bits(lp0)), "z / log_probs were written"
        H, P, C, N = self.H, self.P, self.C, self.N
        for b in (self.gWp, self.gbp, self.gWc, self.gbc, self.loss):
            assert b.same_where(torch.zeros(b.n, dtype=torch.bool))
        assert self.ws.same_where(torch.zeros(self.ws.n, dtype=torch.bool))   # (the whole workspace is the call's; its guards are not)
        ws = self.ws.now()
        g = {"gWp": self.gWp.now().view(H, P).numpy().copy(), "gbp": self.gbp.now().numpy().copy(),
             "gWc": self.gWc.now().view(P, C).numpy().copy(), "gbc": self.gbc.now().numpy().copy(),
             "loss": float(self.loss.now()[0]), "n_valid": int(ws[:1].view(torch.int32)[0]),
             "dpre": ws[64:64 + N * P].view(N, P).numpy().copy()}
        self.grads = g
        return g

    def reference(self):
        d = self.d
        keep, scale = R.keep_mask_seed(self.seed, self.N, self.P, self.p)
        keep = None if self.p == 0.0 else keep
        x = self.gathered()
        f = R.forward(x, d["Wp"], d["bp"], d["Wc"], d["bc"], d["labels"] if self.lab is not None else None, keep, scale)
        fb = R.forward_bounds(x, d["Wp"], d["bp"], d["Wc"], d["bc"], f, keep, scale)
        return x, f, fb, keep, scale


def check_forward(call, tag, cap=True):
    out = call.out
    x, f, fb, keep, scale = call.reference()
    N = call.N
    for k in ("z", "logits", "log_probs", "nll"):
        q = R.ratio(out[k], f[k], fb[k])
        print(f"cls fwd {tag} {k}: {q:.4f} of its bound")
        within(f"cls fwd {k} / bound", q, 1.0, tag)
    pd, rd = R.decided(f, fb)
    left = int((~pd).sum() + (~rd).sum())
    print(f"cls fwd {tag}: {left} of {2 * N} integer outputs left to the bound")
    if cap:
        assert left * 100 <= 2 * N, (tag, left)
    assert np.array_equal(out["pred"][pd], f["pred"][pd]), tag
    assert np.array_equal(out["label_rank"][rd], f["label_rank"][rd]), tag
    # exact statements about the call's own bits
    lg = out["logits"].astype(np.float64)
    assert np.array_equal(out["pred"], np.argmax(lg, axis=1)), "pred is not the first maximum of the call's own logits"
    assert np.array_equal(out["label_rank"], R.label_rank(lg, f["labels"])), "label_rank is not the rule on the call's own logits"
    assert np.all((out["label_rank"] == 0) == ((out["pred"] == f["labels"]) & f["valid"]))
    assert np.all(out["nll"][~f["valid"]] == 0.0) and np.all(out["label_rank"][~f["valid"]] == -1)
    lab = np.where(f["valid"], f["labels"], 0)
    assert np.array_equal(out["nll"][f["valid"]], -out["log_probs"][np.arange(N), lab][f["valid"]])
    return x, f, fb, keep, scale


def check_backward(call, tag, ref):
    x, f, fb, keep, scale = ref
    g = call.grads
    rg = R.backward(x, call.d["Wc"], f, keep, scale)
    gb = R.backward_bounds(x, call.d["Wc"], f, rg, fb, keep, scale)
    assert g["n_valid"] == rg["n_valid"]
    for k in ("loss", "dpre", "gWp", "gbp", "gWc", "gbc"):
        q = R.ratio(g[k], rg[k], gb[k])
        print(f"cls bwd {tag} {k}: {q:.4f} of its bound")
        within(f"cls bwd {k} / bound", q, 1.0, tag)
    return rg


# (N, H, P, C, p, row_index kind, seed): every tail of every axis - N 1, 3, 8, one more than the row tile, two tiles + 1,
# more than one 32-row slice of the outer-product kernel (70), more than one of its 256-row chunks and more than one trip of
# the 256-thread count (300: the fixed-order fold of two chunks); H 4,
# 100, 768 (three 256-column slices); P 2, 62, 130, 256; C 1, 2, 7, 65, 1024.  The worst-case logit bound grows with H P, so
# the widest head goes with few classes: with 65 classes behind H 768, P 256 the float64 logits lie closer together than
# twice the bound in a third of the rows, whatever the seed.
CASES = [
    (1, 4, 2, 1, 0.0, None, 1), (3, 100, 62, 7, 0.1, "reverse", 2), (8, 768, 256, 2, 0.5, None, 3),
    (TR + 1, 100, 130, 65, 0.0, "repeat", 4), (2 * TR + 1, 4, 62, 1024, 0.1, None, 5), (2 * TR + 1, 768, 256, 7, 0.1, "reverse", 6),
    (70, 100, 2, 7, 0.5, "repeat", 7), (300, 4, 62, 2, 0.1, None, 8), (3, 768, 130, 1, 0.5, None, 9),
    (8, 4, 256, 1024, 0.0, "reverse", 29), (1, 100, 256, 65, 0.1, None, 11), (TR + 1, 768, 2, 2, 0.0, None, 12),
    (TR + 1, 4, 1024, 1024, 0.1, None, 13),   # both at their limit: the forward's LDS is exactly 64 KB
]


def make_index(kind, N, rng):
    """(row_index or None, n_src)."""
    if kind is None:
        return None, N
    if kind == "reverse":
        return np.arange(N - 1, -1, -1), N
    n_src = max(2, N // 2 + 1)
    idx = rng.integers(0, n_src, N)
    idx[-1] = idx[0]   # (at least one repeat)
    return idx, n_src


@pytest.mark.parametrize("N,H,P,C,p,kind,seed", CASES)
def test_random_cases_against_float64(dev, N, H, P, C, p, kind, seed):
    rng = np.random.default_rng(1000 + seed)
    idx, n_src = make_index(kind, N, rng)
    d = R.head_inputs(N, H, P, C, seed, n_src=n_src)
    if P == 1024 and C == 1024:
        # 1024 random logits behind a dot product of length 1024 lie closer together than twice its worst-case bound: this
        # case spreads them by the bias (a shuffled grid of step 1 / 64) and keeps the classifier's kernel small
        d["Wc"] = (d["Wc"] * 0.01).astype(np.float32)
        d["bc"] = rng.permutation(np.linspace(-8.0, 8.0, C)).astype(np.float32)
    tag = f"N{N} H{H} P{P} C{C} p{p} {kind}"
    call = Call(dev, d, N, p=p, seed=0xC0FFEE + seed, row_index=idx, confusion=True)
    out = call.fwd()
    ref = check_forward(call, tag)
    f = ref[1]
    want = np.zeros((C, C), dtype=np.int64)
    for r in range(N):
        if f["valid"][r]:
            want[f["labels"][r], out["pred"][r]] += 1
    assert np.array_equal(out["confusion"], want)
    call.bwd()
    check_backward(call, tag, ref)


def test_two_identical_calls_give_identical_bits(dev):
    N, H, P, C = 2 * TR + 1, 100, 62, 65
    d = R.head_inputs(N, H, P, C, 21)
    res = []
    for _ in range(2):
        call = Call(dev, d, N, p=0.1, seed=77, confusion=True)
        out = call.fwd()
        g = call.bwd()
        res.append({**out, **{k: np.asarray(v) for k, v in g.items()}})
    for k in res[0]:
        a, b = np.ascontiguousarray(res[0][k]), np.ascontiguousarray(res[1][k])
        assert a.tobytes() == b.tobytes(), k


def test_rate_zero_ignores_the_seed_and_optional_outputs_are_optional(dev):
    N, H, P, C = TR + 1, 100, 62, 7
    d = R.head_inputs(N, H, P, C, 22)
    a, b = Call(dev, d, N, p=0.0, seed=0), Call(dev, d, N, p=0.0, seed=0x123456789ABCDEF)
    oa, ob = a.fwd(), b.fwd()
    ga, gb = a.bwd(), b.bwd()
    for k in oa:
        assert np.ascontiguousarray(oa[k]).tobytes() == np.ascontiguousarray(ob[k]).tobytes(), k
    for k in ga:
        assert np.asarray(ga[k]).tobytes() == np.asarray(gb[k]).tobytes(), k
    # no optional output, no labels: logits and pred are the same bits
    c = Call(dev, d, N, optional=False, labels=False)
    oc = c.fwd()
    assert oc["logits"].tobytes() == oa["logits"].tobytes() and np.array_equal(oc["pred"], oa["pred"])


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_zero_pattern_of_y_is_the_host_mask(dev, p):
    """Wc = identity, bc = 0: logits[r][c] = fmaf(y[r][c], 1, 0 + ...zeros) = y[r][c] exactly."""
    N, P = 2 * TR + 1, 130
    d = R.head_inputs(N, 100, P, P, 23)
    d["Wc"] = np.eye(P, dtype=np.float32)
    d["bc"] = np.zeros(P, dtype=np.float32)
    call = Call(dev, d, N, p=p, seed=4242)
    out = call.fwd()
    keep, scale = R.keep_mask_seed(4242, N, P, p)
    assert np.all(out["z"] != 0.0)
    assert np.array_equal(out["logits"] != 0.0, keep), "the zero pattern of y is not the host mask"
    assert 0.5 * p < 1.0 - keep.mean() < 1.5 * p
    want = np.where(keep, out["z"] * np.float32(scale), np.float32(0))   # one fp32 multiply of the call's own z
    assert want.astype(np.float32).tobytes() == out["logits"].tobytes()


def test_planted_ties(dev):
    """Wc = 0: the logits are bc exactly, for every row.  Ties inside a lane's own classes (3 and 67), across lanes (3 and 70)
    and between -0 and +0."""
    C, P, H = 130, 2, 4
    bc = np.full(C, -1.0, dtype=np.float32)
    bc[[3, 67, 70]] = 2.5
    bc[[5, 129]] = 1.0
    bc[10], bc[11] = 0.0, -0.0
    labels = np.array([3, 67, 70, 5, 129, 0, 10, 11, -1, 64], dtype=np.int32)
    N = len(labels)
    d = R.head_inputs(N, H, P, C, 24)
    d.update(Wc=np.zeros((P, C), dtype=np.float32), bc=bc, labels=labels)
    call = Call(dev, d, N, confusion=True)
    out = call.fwd()
    assert np.array_equal(out["logits"], np.tile(bc, (N, 1)))   # (numerically: 0 + -0 is +0)
    assert np.all(out["pred"] == 3)
    n_neg_below = lambda k: int((bc[:k] == -1.0).sum())
    assert out["label_rank"].tolist() == [0, 1, 2, 3, 4, 7 + n_neg_below(0), 5, 6, -1, 7 + n_neg_below(64)]
    assert np.array_equal(out["label_rank"], R.label_rank(np.tile(bc, (N, 1)), labels))
    want = np.zeros((C, C), dtype=np.int64)
    for lab in labels[labels >= 0]:
        want[lab, 3] += 1
    assert np.array_equal(out["confusion"], want)
    out2 = call.fwd()                      # the same table passed in again: accumulated on the device
    assert np.array_equal(out2["confusion"], 2 * want)


def test_saturated_tanh_and_large_logits(dev):
    """Pre-activations of +-20: tanhf gives +-1 exactly, so 1 - z^2 and with it dpre, gWp and gbp are exactly 0.  Logits
    of +-80: the softmax saturates (exp(-160) underflows to 0)."""
    N, H, P, C = TR + 1, 100, 62, 7
    d = R.head_inputs(N, H, P, C, 25)
    d["Wp"] = np.zeros((H, P), dtype=np.float32)
    d["bp"] = np.where(np.arange(P) % 2 == 0, 20.0, -20.0).astype(np.float32)
    d["bc"] = np.array([80.0, -80.0, 0.0, 80.0, -80.0, 1.0, -1.0], dtype=np.float32)
    d["Wc"] = (d["Wc"] * 0.01).astype(np.float32)
    call = Call(dev, d, N, p=0.1, seed=99)
    out = call.fwd()
    assert out["z"].tobytes() == np.tile(np.where(np.arange(P) % 2 == 0, 1.0, -1.0).astype(np.float32), (N, 1)).tobytes()
    ref = check_forward(call, "saturated", cap=False)
    assert np.all(np.isin(out["pred"], (0, 3)))
    g = call.bwd()
    check_backward(call, "saturated", ref)
    assert np.all(g["dpre"] == 0.0) and np.all(g["gWp"] == 0.0) and np.all(g["gbp"] == 0.0)
    assert np.any(g["gWc"] != 0.0) and np.isfinite(g["loss"])


@pytest.mark.parametrize("labelled", [0, 1])
def test_unlabelled_rows(dev, labelled):
    N, H, P, C = 2 * TR + 1, 100, 62, 7
    d = R.head_inputs(N, H, P, C, 26)
    lab = np.full(N, -1, dtype=np.int32)
    lab[1], lab[5] = C, -7                 # (outside [0, C) on either side: unlabelled too)
    if labelled:
        lab[TR + 2] = 4
    d["labels"] = lab
    call = Call(dev, d, N, p=0.1, seed=5, confusion=True)
    out = call.fwd()
    ref = check_forward(call, f"unlabelled+{labelled}")
    assert int(out["confusion"].sum()) == labelled
    g = call.bwd()
    check_backward(call, f"unlabelled+{labelled}", ref)
    assert g["n_valid"] == labelled
    if not labelled:
        assert g["loss"] == 0.0 and all(np.all(g[k] == 0.0) for k in ("gWp", "gbp", "gWc", "gbc", "dpre"))
    else:
        rows = np.arange(N) != TR + 2
        assert np.all(g["dpre"][rows] == 0.0) and g["loss"] == out["nll"][TR + 2]


def test_an_index_outside_the_source_reads_zeros(dev):
    N, H, P, C = 3, 100, 62, 7
    d = R.head_inputs(N, H, P, C, 27, n_src=2)
    call = Call(dev, d, N, row_index=[1, 5, -1])
    out = call.fwd()
    d0 = dict(d, x=np.concatenate([d["x"], np.zeros((1, H), dtype=np.float32)]))
    ref = Call(dev, d0, N, row_index=[1, 2, 2]).fwd()
    assert out["logits"].tobytes() == ref["logits"].tobytes()


def test_limits_are_refused_with_nothing_written(dev):
    lib = _L().lib()
    N, H, P, C = 3, 8, 4, 3
    d = R.head_inputs(N, H, P, C, 28)
    call = Call(dev, d, N, confusion=True)
    call.fwd()
    call.bwd()
    outs = [call.logits, call.pred, call.z, call.lp, call.nll, call.rank, call.conf, call.gWp, call.gbp, call.gWc, call.gbc,
            call.loss, call.ws]
    for b in outs:
        b.host0 = b.t.cpu()               # (the state after the valid calls: nothing may move from here on)
    F = {n: i for i, n in enumerate(("x", "ld_x", "n_src", "idx", "Wp", "bp", "Wc", "bc", "lab", "p", "seed", "logits", "ld_lg",
                                     "pred", "z", "ld_z", "lp", "ld_lp", "nll", "rank", "conf", "ld_cf", "N", "H", "P", "C"))}
    B = {n: i for i, n in enumerate(("x", "ld_x", "n_src", "idx", "Wc", "lab", "p", "seed", "z", "ld_z", "lp", "ld_lp", "gWp", "gbp",
                                     "gWc", "gbc", "loss", "ws", "ws_bytes", "N", "H", "P", "C"))}
    bad = [("N", 0), ("N", 65536), ("H", 4100), ("H", 6), ("H", 0), ("P", 3), ("P", 1026), ("P", 0), ("C", 0), ("C", 1025),
           ("p", 1.0), ("p", -0.1), ("ld_x", H - 1), ("n_src", 0), ("n_src", N - 1)]
    for name, v in bad + [("ld_lg", C - 1), ("ld_z", P - 1), ("ld_lp", C - 1), ("ld_cf", C - 1), ("logits", None), ("pred", None),
                          ("x", None), ("Wp", None), ("bc", None), ("x", call.X.v.data_ptr() + 2)]:
        a = call.fwd_args()
        a[F[name]] = v
        assert lib.tmi_cls_head_fwd(*a) == TMI_ERR_INVALID, ("fwd", name, v)
        assert b"tmi_cls_head_fwd" in lib.tmi_last_error()
    for name, v in bad + [("ld_z", P - 1), ("ld_lp", C - 1), ("ws_bytes", call.ws.n * 4 - 4), ("ws", None), ("lab", None), ("z", None),
                          ("gWp", None), ("loss", None), ("ws", call.ws.v.data_ptr() + 4)]:
        a = call.bwd_args()
        a[B[name]] = v
        assert lib.tmi_cls_head_bwd(*a) == TMI_ERR_INVALID, ("bwd", name, v)
        assert b"tmi_cls_head_bwd" in lib.tmi_last_error()
    for n, h, p_, c in ((0, H, P, C), (65536, H, P, C), (N, 6, P, C), (N, 4100, P, C), (N, H, 3, C), (N, H, 1026, C), (N, H, P, 0),
                        (N, H, P, 1025)):
        assert lib.tmi_cls_head_workspace_bytes(n, h, p_, c) == -1
    torch.cuda.synchronize()
    for b in outs + call.inputs:
        assert b.same_where(), "a refused call wrote something"
