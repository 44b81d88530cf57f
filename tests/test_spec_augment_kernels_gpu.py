"""tmi_spec_masks, tmi_span_mask_apply (csrc/spec_augment.hip) and the masked forms tmi_ctc_head_fwd_m, tmi_ctc_head_bwd_m,
tmi_layer_mix_bwd_m, with no tolerance anywhere.

The masks are compared bit for bit with tests/_spec_augment_ref.py (checked by tests/test_spec_augment_cpu.py): N 1 / 3 / 5,
T_max 1 .. 200 over the word and wave edges, H 8 / 72 / 264 / 1024, length 1 .. 64, prob 0 .. 0.999, ld at its minimum and
padded, each pointer NULL in turn, counts against the popcounts, two calls giving equal bits.  Every buffer lies inside
guard zones (7 / a large negative, 7.0 / NaN) in the style of tests/test_layer_mix_kernels_gpu.py: the guards, the stride
padding and the inputs are what they were, and so is everything after a refused call.

The fusion: each masked call on x gives bit for bit what the EXISTING entry point gives on x', x with the masked elements set
to +0 on the host and gathered by position (fmaf(0, w, acc) == acc on these chains from +0, so no bound is needed)."""
import numpy as np
import pytest
import torch

import _ctc_ref as C
import _spec_augment_ref as S

pytestmark = pytest.mark.gpu

F32, I32, BF16 = torch.float32, torch.int32, torch.bfloat16
TMI_ERR_INVALID = -1
PAD = 64


def _lib():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib as L
    return L.lib()


def _ops():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops
    return ops


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def stream():
    return torch.cuda.current_stream().cuda_stream


class G:
    """``n`` payload elements inside guards; ``v`` is the payload on the device."""

    def __init__(self, dev, dtype, n, fill=None):
        host = C.guard_pattern(n + 2 * PAD, F32 if dtype == BF16 else dtype).to(dtype)
        if fill is not None:
            fill(host[PAD:PAD + n])
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


# ================================================================================================ tmi_spec_masks
class Masks:
    def __init__(self, dev, N, T, H, pad_t=0, pad_f=0, time=True, feat=True, counts=True):
        self.N, self.T, self.H = N, T, H
        self.ld_t, self.ld_f = S.words(T) + pad_t, S.words(H) + pad_f
        self.tb = G(dev, I32, N * self.ld_t) if time else None
        self.fb = G(dev, I32, N * self.ld_f) if feat else None
        self.cnt = G(dev, I32, 2 * N) if counts else None

    def args(self, tp, tl, fp, fl, seed, **over):
        p = lambda g: None if g is None else g.v.data_ptr()
        a = dict(time_bits=p(self.tb), ld_t=self.ld_t, feat_bits=p(self.fb), ld_f=self.ld_f, counts=p(self.cnt), N=self.N,
                 T_max=self.T, H=self.H, time_prob=tp, time_length=tl, feat_prob=fp, feat_length=fl, seed=seed, stream=stream())
        a.update(over)
        return list(a.values())

    def got(self, g, ld):
        return g.now().numpy().view(np.uint32).reshape(self.N, ld)

    def unwritten(self, ld, cols):
        k = torch.ones((self.N, ld), dtype=torch.bool)
        k[:, :S.words(cols)] = False
        return k

    def check(self, tp, tl, fp, fl, seed):
        """One call against the restatement; -> the bits of everything the call owns."""
        lib = _lib()
        assert lib.tmi_spec_masks(*self.args(tp, tl, fp, fl, seed)) == 0, lib.tmi_last_error()
        torch.cuda.synchronize()
        tm, fm = S.time_mask(seed, self.N, self.T, tp, tl), S.feature_mask(seed, self.N, self.H, fp, fl)
        out = []
        for g, ld, cols, m in ((self.tb, self.ld_t, self.T, tm), (self.fb, self.ld_f, self.H, fm)):
            if g is None:
                continue
            w = S.words(cols)
            assert np.array_equal(self.got(g, ld)[:, :w], S.pack_bits(m)), "the bits differ from the restatement"
            assert g.same_where(self.unwritten(ld, cols)), "a word past ceil(cols / 32) or a guard was written"
            out.append(bits(g.t))
        if self.cnt is not None:
            want = np.stack([tm.sum(1) if self.tb is not None else 0 * tm.sum(1), fm.sum(1) if self.fb is not None else 0 * fm.sum(1)], 1)
            assert np.array_equal(self.cnt.now().numpy().reshape(self.N, 2), want.astype(np.int32)), "counts are not the popcounts"
            assert self.cnt.same_where(torch.zeros(2 * self.N, dtype=torch.bool))
            out.append(bits(self.cnt.t))
        return torch.cat(out)


LENGTHS = [1, 2, 10, 32, 33, 64]
PROBS = [0.0, 0.05, 0.5, 0.999]


@pytest.mark.parametrize("T_max", [1, 31, 32, 33, 63, 64, 65, 129, 200])
def test_masks_equal_the_restatement_bit_for_bit(dev, T_max):
    i = 0
    for length in LENGTHS:
        for prob in PROBS:
            N, H = (1, 3, 5)[i % 3], (8, 72, 264, 1024)[(i // 3) % 4]
            m = Masks(dev, N, T_max, H, pad_t=(i % 2) * 3, pad_f=((i + 1) % 2) * 2)
            # the feature mask takes the other end of the two lists, so every (length, prob) pair meets every H over the T_max cases
            fl, fp = LENGTHS[(i + T_max) % 6], PROBS[(i // 2 + T_max) % 4]
            seed = S.site_seed(1000 + T_max, i)
            first = m.check(prob, length, fp, fl, seed)
            assert torch.equal(first, m.check(prob, length, fp, fl, seed)), "two calls gave different bits"
            i += 1


@pytest.mark.parametrize("H", [8, 72, 264, 1024])
def test_feature_mask_over_every_length_and_rate(dev, H):
    for j, length in enumerate(LENGTHS):
        for k, prob in enumerate(PROBS):
            Masks(dev, (5, 1, 3)[(j + k) % 3], 40, H, pad_f=k % 2).check(0.05, 10, prob, length, S.site_seed(H, 6 * j + k))


def test_each_pointer_may_be_null(dev):
    N, T, H, seed = 3, 129, 264, S.site_seed(3, 4)
    both = Masks(dev, N, T, H)
    both.check(0.5, 10, 0.05, 33, seed)
    only_t, only_f = Masks(dev, N, T, H, feat=False), Masks(dev, N, T, H, time=False)
    # (the prob / length / ld of a mask that is off are not looked at)
    lib = _lib()
    assert lib.tmi_spec_masks(*only_t.args(0.5, 10, 7.0, 0, seed, ld_f=0)) == 0, lib.tmi_last_error()
    assert lib.tmi_spec_masks(*only_f.args(-1.0, 99, 0.05, 33, seed, ld_t=0)) == 0, lib.tmi_last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(only_t.tb.t), bits(both.tb.t)) and torch.equal(bits(only_f.fb.t), bits(both.fb.t))
    c = both.cnt.now().reshape(N, 2)
    assert torch.equal(only_t.cnt.now().reshape(N, 2), torch.stack([c[:, 0], torch.zeros(N, dtype=I32)], 1))
    assert torch.equal(only_f.cnt.now().reshape(N, 2), torch.stack([torch.zeros(N, dtype=I32), c[:, 1]], 1))
    bare = Masks(dev, N, T, H, counts=False)
    assert torch.equal(bare.check(0.5, 10, 0.05, 33, seed), torch.cat([bits(both.tb.t), bits(both.fb.t)]))


def test_refused_mask_calls_write_nothing(dev):
    m = Masks(dev, 3, 65, 72, pad_t=1)
    lib = _lib()
    ok = dict(tp=0.05, tl=10, fp=0.05, fl=10, seed=5)
    for over in (dict(time_length=0), dict(time_length=65), dict(feat_length=0), dict(feat_length=65), dict(time_prob=-0.01),
                 dict(time_prob=1.0), dict(feat_prob=1.0), dict(feat_prob=-1.0), dict(N=0), dict(N=65536), dict(T_max=0),
                 dict(T_max=4097), dict(H=12), dict(H=0), dict(ld_t=S.words(65) - 1), dict(ld_f=S.words(72) - 1),
                 dict(time_bits=None, feat_bits=None), dict(time_bits=m.tb.v.data_ptr() + 2), dict(counts=m.cnt.v.data_ptr() + 2)):
        assert lib.tmi_spec_masks(*m.args(**ok, **over)) == TMI_ERR_INVALID, over
        msg = lib.tmi_last_error().decode()
        assert msg.startswith("tmi_spec_masks:") and "1 <= length <= 64" in msg and "0 <= prob < 1" in msg, msg
    torch.cuda.synchronize()
    assert m.tb.same_where() and m.fb.same_where() and m.cnt.same_where()


# ================================================================================================ tmi_span_mask_apply
def strided(dev, a, st, sn, dtype):
    """a [n, T, c] as a device view with frame stride ``st`` and item stride ``sn`` inside a guard buffer -> (G, view)."""
    n, T, c = a.shape
    g = G(dev, dtype, n * sn)
    v = torch.as_strided(g.v, (n, T, c), (sn, st, 1))
    v.copy_(torch.as_tensor(a).to(dev, dtype))
    g.host0 = g.t.cpu().clone()
    return g, v


def dev_bits(dev, mask, pad=0):
    """bool [N, cols] -> the int32 device tensor [N, words + pad] tmi_spec_masks would have written."""
    return torch.from_numpy(S.pack_bits(mask, S.words(mask.shape[1]) + pad).view(np.int32)).to(dev)


@pytest.mark.parametrize("x_pad", [0, 8, 1])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_span_mask_apply_equals_where(dev, dtype, x_pad):
    ops = _ops()
    N, T, H = 3, 37, 72
    g = np.random.default_rng(11 + x_pad)
    x = torch.from_numpy(g.standard_normal((N, T, H)).astype(np.float32)).to(dtype)
    x[0, 0, :4] = torch.tensor([float("nan"), float("inf"), -0.0, -1.0]).to(dtype)
    tm, fm = S.time_mask(9, N, T, 0.2, 3), S.feature_mask(9, N, H, 0.1, 5)
    tm[1, :] = True
    st = H + x_pad
    gx, xv = strided(dev, x, st, T * st + (16 if x_pad % 8 == 0 else 5), dtype)
    o_st = H + (8 if x_pad % 8 == 0 else 3)
    for tmask, fmask in ((tm, fm), (tm, None), (None, fm), (None, None)):
        go, ov = strided(dev, torch.zeros((N, T, H)), o_st, T * o_st + (8 if x_pad % 8 == 0 else 1), dtype)
        go = G(dev, dtype, go.n)   # (a fresh guard pattern: the call must write every payload element of the view)
        ov = torch.as_strided(go.v, (N, T, H), (ov.stride(0), o_st, 1))
        ops.span_mask_apply(xv, ov, None if tmask is None else dev_bits(dev, tmask, 1), None if fmask is None else dev_bits(dev, fmask))
        torch.cuda.synchronize()
        full = torch.zeros((N, T, H), dtype=torch.bool)
        if tmask is not None:
            full |= torch.from_numpy(tmask)[:, :, None]
        if fmask is not None:
            full |= torch.from_numpy(fmask)[:, None, :]
        want = torch.where(full, torch.zeros((), dtype=dtype), x)
        assert torch.equal(bits(ov), bits(want)), "out != where(mask, +0, x) bit for bit"
        written = torch.zeros(go.n, dtype=torch.bool)
        torch.as_strided(written, (N, T, H), (ov.stride(0), o_st, 1)).fill_(True)
        assert go.same_where(~written) and gx.same_where(), "the padding, a guard or the input was written"
    lib = _lib()
    for over in (dict(H=12), dict(x_dtype=2), dict(x_st=H - 1), dict(o_st=H - 1), dict(ld_t=S.words(T) - 1), dict(N=0), dict(out=None)):
        a = dict(x=xv.data_ptr(), x_dtype=1 if dtype == BF16 else 0, x_sn=xv.stride(0), x_st=st, time_bits=dev_bits(dev, tm).data_ptr(),
                 ld_t=S.words(T), feat_bits=None, ld_f=0, out=ov.data_ptr(), o_sn=ov.stride(0), o_st=o_st, N=N, T=T, H=H, stream=stream())
        a.update(over)
        before = bits(go.t)
        assert lib.tmi_span_mask_apply(*a.values()) == TMI_ERR_INVALID, over
        assert lib.tmi_last_error().decode().startswith("tmi_span_mask_apply:")
        torch.cuda.synchronize()
        assert torch.equal(bits(go.t), before)


# ================================================================================================ the fusion
L_MAX = 6
# name: (N, T_max, H, V, K, dtype, p, reduction, x_pad, permuted row_index): the smallest hard cases of the head and mix tests
FUSION = {
    "R350 H264 V33 K13 bf16 perm": (5, 70, 264, 33, 13, BF16, 0.1, "mean", 8, True),
    "H72 V31 K2 f32": (3, 37, 72, 31, 2, F32, 0.0, "sum", 3, False),
    "R8193 H8 V2 K2 bf16": (3, 2731, 8, 2, 2, BF16, 0.1, "sum", 0, False),
    "H72 V64 K13 bf16 perm odd stride": (4, 20, 72, 64, 13, BF16, 0.1, "mean", 1, True),
    "H8 V2 K2 f32 perm": (3, 9, 8, 2, 2, F32, 0.0, "mean", 8, True),
}
_CASES = {}


def fusion_case(name):
    """The seeded host inputs of a case and its masks (computed once, nobody writes into them)."""
    if name in _CASES:
        return _CASES[name]
    N, T, H, V, K, dtype, p, reduction, x_pad, perm = FUSION[name]
    g = np.random.default_rng(sum(map(ord, name)))
    n_src = N + 2
    layers = torch.from_numpy(g.standard_normal((K, n_src, T, H)).astype(np.float32)).to(dtype)
    row_index = None
    if perm:
        row_index = g.permutation(n_src)[:N].astype(np.int32)
        row_index[N // 2] = n_src + 3                      # out of range: reads as zeros
    frame_lens = g.integers(max(1, T // 2), T + 1, N).astype(np.int32)
    frame_lens[0], frame_lens[1], frame_lens[2] = T, T + 5, 0   # full, beyond T_max (clamped), empty
    infeasible = np.zeros(N, dtype=np.int32)
    infeasible[N - 1] = 1
    tm, fm = S.time_mask(S.site_seed(7, 1), N, T, 0.2, 3), S.feature_mask(S.site_seed(7, 1), N, H, 0.1, 5)
    tm[0, :] = True                                        # a fully time-masked item (a live one: frame_lens[0] = T)
    assert tm[1].any() and not tm[1].all() and fm.any() and not fm.all(axis=1).any()
    _CASES[name] = dict(
        N=N, T=T, H=H, V=V, K=K, dtype=dtype, p=p, reduction=reduction, x_st=H + x_pad, n_src=n_src, layers=layers, row_index=row_index,
        frame_lens=frame_lens, label_lens=g.integers(0, L_MAX + 1, N).astype(np.int32), infeasible=infeasible,
        W=(g.uniform(-1, 1, (H, V)) * np.sqrt(6.0 / (H + V)) * 2.0).astype(np.float32), b=(g.standard_normal(V) * 0.5).astype(np.float32),
        a=(g.standard_normal(K) * 1.5).astype(np.float32), grad=(g.standard_normal((N, T, V)) * 0.3).astype(np.float32),
        nll=g.uniform(1.0, 30.0, N).astype(np.float32), tm=tm, fm=fm, seed=4242)
    return _CASES[name]


def premasked(d, tmask, fmask):
    """x': the K layers gathered by position (an index out of range: zeros) with the masked elements set to +0."""
    x = d["layers"]
    if d["row_index"] is not None:
        idx = torch.from_numpy(d["row_index"]).long()
        ok = (idx >= 0) & (idx < d["n_src"])
        x = torch.where(ok[None, :, None, None], x[:, idx.clamp(0, d["n_src"] - 1)], torch.zeros((), dtype=x.dtype))
    else:
        x = x[:, :d["N"]].clone()
    full = torch.zeros(x.shape[1:], dtype=torch.bool)
    if tmask is not None:
        full |= torch.from_numpy(tmask)[:, :, None]
    if fmask is not None:
        full |= torch.from_numpy(fmask)[:, None, :]
    return torch.where(full[None], torch.zeros((), dtype=x.dtype), x)


def run_head_and_mix(dev, d, layers, n_src, row_index, tb, fb):
    """The three calls that read the features on one set of layers -> every output, as bits.  The head reads the last layer
    directly (through row_index) and, as the mixed step does, the mix of all layers by position."""
    ops = _ops()
    N, T, H, V, K = d["N"], d["T"], d["H"], d["V"], d["K"]
    st = d["x_st"]
    sn = T * st + (16 if st % 8 == 0 else 5)
    keep = [strided(dev, layers[k], st, sn, d["dtype"]) for k in range(K)]
    X = [v for _, v in keep]
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    idx, fl, ll, bad = to(row_index), to(d["frame_lens"]), to(d["label_lens"]), to(d["infeasible"])
    W, b, a, grad, nll = to(d["W"]), to(d["b"]), to(d["a"]), to(d["grad"]), to(d["nll"])
    z = lambda *s, dt=F32: torch.zeros(s, dtype=dt, device=dev)
    out = {}
    mixed = z(N, T, H)
    ops.layer_mix_fwd(X, a, fl, mixed, row_index=idx)
    for tag, hidden, ri in (("last", X[K - 1], idx), ("mixed", mixed, None)):
        logp, logits, amax = z(N, T, V), z(N, T, V), z(N, T, dt=I32)
        ops.ctc_head_fwd(hidden, W, b, fl, logp, row_index=ri, p=d["p"], seed=d["seed"], logits=logits, argmax=amax, time_bits=tb,
                         feat_bits=fb)
        gW, gb, loss, n_bad = z(H, V), z(V), z(1), z(1, dt=I32)
        ws = torch.empty(ops.ctc_head_workspace_elems(N, T, H, V), dtype=F32, device=dev)
        ops.ctc_head_bwd(hidden, fl, ll, grad, nll, bad, gW, gb, loss, n_bad, ws, L_MAX, row_index=ri, p=d["p"], seed=d["seed"],
                         reduction=d["reduction"], time_bits=tb, feat_bits=fb)
        out.update({f"{tag} {k}": v for k, v in dict(logp=logp, logits=logits, argmax=amax, gW=gW, gb=gb, loss=loss,
                                                      n_infeasible=n_bad).items()})
    g_a, dk = z(K), z(K)
    ws = torch.empty(ops.layer_mix_workspace_elems(N, T, H, V, K), dtype=F32, device=dev)
    ops.layer_mix_bwd(X, a, fl, ll, grad, bad, W, g_a, ws, L_MAX, row_index=idx, p=d["p"], seed=d["seed"], reduction=d["reduction"],
                      d=dk, time_bits=tb, feat_bits=fb)
    out.update(g_a=g_a, d=dk)
    torch.cuda.synchronize()
    for gbuf, _ in keep:
        assert gbuf.same_where(), "an input layer was written"
    return {k: bits(v) for k, v in out.items()}, out


def compare(got, want, tag):
    for k in want:
        assert torch.equal(got[k], want[k]), f"{tag}: {k} differs from the existing call on the pre-masked copy"


@pytest.mark.parametrize("name", list(FUSION))
def test_masked_calls_equal_the_existing_calls_on_a_premasked_copy(dev, name):
    d = fusion_case(name)
    tb, fb = dev_bits(dev, d["tm"], 1), dev_bits(dev, d["fm"])
    got, raw = run_head_and_mix(dev, d, d["layers"], d["n_src"], d["row_index"], tb, fb)
    want, _ = run_head_and_mix(dev, d, premasked(d, d["tm"], d["fm"]), d["N"], None, None, None)
    compare(got, want, name)
    # the masks did something, and a time-masked live row's logits are the bias
    plain, _ = run_head_and_mix(dev, d, d["layers"], d["n_src"], d["row_index"], None, None)
    assert not torch.equal(plain["last gW"], got["last gW"]) and not torch.equal(plain["d"], got["d"])
    assert torch.equal(raw["last logits"][0].cpu(), torch.from_numpy(d["b"]).expand(d["T"], d["V"]))
    assert torch.isfinite(raw["g_a"]).all() and raw["last gb"].abs().sum() > 0


@pytest.mark.parametrize("which", ["time", "feature"])
@pytest.mark.parametrize("p, reduction", [(0.0, "sum"), (0.1, "mean"), (0.1, "sum"), (0.0, "mean")])
def test_one_mask_alone_every_rate_and_reduction(dev, which, p, reduction):
    d = dict(fusion_case("R350 H264 V33 K13 bf16 perm"), p=p, reduction=reduction)
    tm, fm = (d["tm"], None) if which == "time" else (None, d["fm"])
    got, _ = run_head_and_mix(dev, d, d["layers"], d["n_src"], d["row_index"], None if tm is None else dev_bits(dev, tm),
                              None if fm is None else dev_bits(dev, fm, 2))
    want, _ = run_head_and_mix(dev, d, premasked(d, tm, fm), d["N"], None, None, None)
    compare(got, want, (which, p, reduction))


def test_both_masks_null_is_the_existing_call(dev, monkeypatch):
    d = fusion_case("H72 V64 K13 bf16 perm odd stride")
    want, _ = run_head_and_mix(dev, d, d["layers"], d["n_src"], d["row_index"], None, None)
    lib = _lib()
    calls = []
    for name in ("tmi_ctc_head_fwd", "tmi_ctc_head_bwd", "tmi_layer_mix_bwd"):
        def through_m(*a, _m=getattr(lib, name + "_m"), _name=name):
            calls.append(_name)
            return _m(*a[:-1], None, 0, None, 0, a[-1])
        monkeypatch.setattr(lib, name, through_m)
    got, _ = run_head_and_mix(dev, d, d["layers"], d["n_src"], d["row_index"], None, None)
    assert calls == ["tmi_ctc_head_fwd", "tmi_ctc_head_bwd"] * 2 + ["tmi_layer_mix_bwd"]
    compare(got, want, "NULL masks")


def test_refused_masked_calls(dev):
    """A bad mask argument: TMI_ERR_INVALID naming the masked form, nothing written."""
    ops = _ops()
    d = fusion_case("H8 V2 K2 f32 perm")
    N, T, H, V = d["N"], d["T"], d["H"], d["V"]
    x = d["layers"][0].to(dev)
    fl = torch.from_numpy(d["frame_lens"]).to(dev)
    logp = G(dev, F32, N * T * V)
    view = logp.v.view(N, T, V)
    W, b = torch.from_numpy(d["W"]).to(dev), torch.from_numpy(d["b"]).to(dev)
    tb = dev_bits(dev, d["tm"])
    lib = _lib()
    base = [x.data_ptr(), 0, x.stride(0), x.stride(1), d["n_src"], None, fl.data_ptr(), W.data_ptr(), b.data_ptr(), 0.0, 0, None, 0, 0,
            view.data_ptr(), T * V, V, None, N, T, H, V]
    for masks in ((tb.data_ptr(), 0, None, 0), (tb.data_ptr() + 2, 1, None, 0), (None, 0, tb.data_ptr(), 0), (tb.data_ptr(), 1 << 31, None, 0)):
        assert lib.tmi_ctc_head_fwd_m(*base, *masks, stream()) == TMI_ERR_INVALID, masks
        assert lib.tmi_last_error().decode().startswith("tmi_ctc_head_fwd_m:")
    torch.cuda.synchronize()
    assert logp.same_where()
    with pytest.raises(ValueError, match="time_bits"):
        ops.ctc_head_fwd(x, W, b, fl, view, time_bits=tb[:, :0])
