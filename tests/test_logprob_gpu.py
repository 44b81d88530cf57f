"""tmi_logprob_fold through ``ops`` on logits the test writes itself: argmax and ties are exact, lse and the target
log-probability are held to REL * (scale + |lse|) of the fp64 restatement (tests/_eval_ref.py; the bound form of
tests/_sample_ref.py, scale = the row's largest |logit| - for the recomputed bf16 target also sum_k |x_k w_kt|)."""
import numpy as np
import pytest
import torch

import _eval_ref as E
from _margins import within

pytestmark = pytest.mark.gpu

# Bound on |lse - lse64| and |logprob - logprob64| relative to (scale + |lse|).  Measured on an MI355X over every case of
# test_fold_matches_fp64: lse 8.8e-8, logprob 8.8e-8 (the sums are 64 lane partials of at most 102 vectors each, folded
# as a tree: the error grows like the depth, not like V); the bound is about twice that.
REL = 1.8e-7
D_LM = 40  # reduction length of the recomputed target logit (not a multiple of the wave: a ragged last trip)
MODES = ("fp32", "bf16", "bf16_stored")  # bf16: target logit recomputed from (x, w); bf16_stored: read from the chunk


def _nc():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops
    return ops.logprob_chunk_cols()


def _shapes():
    nc = 8192  # (the library constant; test_chunk_width_is_the_one_the_shapes_assume pins it)
    return [(7, 8), (nc - 1, nc), (nc, nc), (nc + 5, nc + 8), (2 * nc, 2 * nc), (51865, 51904)]


def test_chunk_width_is_the_one_the_shapes_assume(dev):
    assert _nc() == 8192


_CASES = {}


def _case(M, V, ld, mode):
    """Host tensors of one case, built once: logits [M, ld] in the storage dtype (zero pad columns), targets, the LM
    operands (bf16 mode) and the fp64 reference."""
    key = (M, V, ld, mode)
    if key in _CASES:
        return _CASES[key]
    nc = 8192
    g = torch.Generator().manual_seed(1000 * M + V % 997 + len(mode))
    dt = torch.float32 if mode == "fp32" else torch.bfloat16
    x = w = None
    if mode == "bf16":
        x = (torch.randn(M, D_LM, generator=g) * 1.5).to(dt)
        w = torch.zeros(D_LM, ld)
        w[:, :V] = torch.randn(D_LM, V, generator=g) * 0.6
        if M > 1 and V > 16:  # row 1's target (column V // 3) dominates its row: the case the recomputed target exists for
            w[:, V // 3] = 8.0 * x[1].float() / x[1].float().norm()
        w = w.to(dt)
        z = (x.double() @ w.double()).to(dt)
    else:
        z = (torch.randn(M, ld, generator=g) * 3.0).to(dt)
    z[:, V:] = 0
    far = V - 1  # a column of the last chunk
    # (the hard rows are written into stored logits; with operands given the logits stay x . w - a stored target logit that
    # disagrees with its own operands by more than a rounding is not an input the LM head can produce)
    for r in range(M if mode != "bf16" else 0):
        kind, flip = r % 6, (r // 6) % 2
        if kind == 1:    # one spike of +80 among zeros
            z[r, :V] = 0
            z[r, far if flip else min(3, V - 1)] = 80.0
        elif kind == 2:  # all equal
            z[r, :V] = 1.25
        elif kind == 3:  # everything at the mask constant except one 0
            z[r, :V] = -1e4
            z[r, V // 2] = 0.0
        elif kind == 4:  # the maximum in chunk 0 and again in the last chunk: the smaller column wins
            z[r, min(5, V - 1)] = 40.0
            z[r, far] = 40.0
        elif kind == 5:  # -0.0 against +0.0, in either order
            z[r, :V] = -1.0
            a, b = min(2, V - 1), far
            z[r, a], z[r, b] = (0.0, -0.0) if flip else (-0.0, 0.0)
    cols = [0, nc - 1, nc, V - 1, -1, int(torch.randint(0, V, (1,), generator=g))]
    targets = torch.tensor([min(cols[r % 6], V - 1) for r in range(M)], dtype=torch.int32)
    if mode == "bf16" and M > 1 and V > 16:
        targets[1] = V // 3
    zt = None
    scale = z[:, :V].double().abs().max(dim=1).values.numpy()
    scale_lp = scale.copy()
    if mode == "bf16":
        t = targets.clamp(min=0).long()
        wt = w.double()[:, t].t()                        # [M, d]
        zt = (x.double() * wt).sum(dim=1).numpy()
        scale_lp = np.maximum(scale, (x.double().abs() * wt.abs()).sum(dim=1).numpy())
    lse, arg, lp = E.fold(z.double().numpy(), V, targets.numpy(), zt=zt)
    _CASES[key] = dict(z=z, targets=targets, x=x, w=w, lse=lse, arg=arg, lp=lp, scale=scale, scale_lp=scale_lp)
    return _CASES[key]


def _run(dev, c, M, V, ld, pad=None, state_fill=None, nc=None):
    from tethys_speech_amd import ops
    z = c["z"].clone()
    if pad is not None:
        z[:, V:] = pad
    z = z.to(dev)
    lm = None
    if c["x"] is not None:
        xd, wd = c["x"].to(dev), c["w"].to(dev)
        lm = (xd, D_LM, wd, ld, 1, D_LM)
    state = torch.empty(ops.logprob_state_elems(M), dtype=torch.int64, device=dev)
    if state_fill is not None:
        state.view(torch.uint8).fill_(state_fill)
    lse = torch.full((M,), float("nan"), device=dev)
    lp = torch.full((M,), float("nan"), device=dev)
    arg = torch.full((M,), -7, dtype=torch.int32, device=dev)
    ops.logprob_from_logits(z, V, c["targets"].to(dev), state, lse, lp, arg, nc=nc, lm=lm)
    torch.cuda.synchronize()
    return lse.cpu(), lp.cpu(), arg.cpu()


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("V,ld", _shapes())
@pytest.mark.parametrize("M", [1, 3, 17, 65])
def test_fold_matches_fp64(dev, M, V, ld, mode):
    """Every shape and storage mode: argmax exact, lse and logprob within REL, unscored rows exactly 0; pad columns
    [V, ld) holding +3e38 or NaN change no output bit."""
    c = _case(M, V, ld, mode)
    got = _run(dev, c, M, V, ld)
    lse, lp, arg = (t.double().numpy() for t in got)
    assert (arg.astype(np.int64) == c["arg"]).all(), (arg, c["arg"])
    t = c["targets"].numpy()
    assert (lp[t < 0] == 0.0).all() and np.isfinite(lse).all() and np.isfinite(lp).all()
    e_lse = float((np.abs(lse - c["lse"]) / (c["scale"] + np.abs(c["lse"]))).max())
    e_lp = float((np.abs(lp - c["lp"]) / (c["scale_lp"] + np.abs(c["lse"]))).max())
    print(f"logprob_fold {mode} M{M} V{V}: |lse - lse64| / (scale + |lse|) = {e_lse:.3e}, logprob {e_lp:.3e}")
    within(f"logprob_fold {mode} |lse - lse64| / (scale + |lse|)", e_lse, REL)
    within(f"logprob_fold {mode} |logprob - logprob64| / (scale + |lse|)", e_lp, REL)
    if ld > V:
        for pad in (3e38, float("nan")):
            assert _same_bits(got, _run(dev, c, M, V, ld, pad=pad)), pad


@pytest.mark.parametrize("mode", MODES)
def test_bit_reproducible_and_state_needs_no_initialisation(dev, mode):
    M, V, ld = 17, 8192 + 5, 8192 + 8  # two chunks: the second folds into stored state
    c = _case(M, V, ld, mode)
    a = _run(dev, c, M, V, ld, state_fill=0)
    assert _same_bits(a, _run(dev, c, M, V, ld, state_fill=0))
    assert _same_bits(a, _run(dev, c, M, V, ld, state_fill=0xFF))  # garbage (NaN bit patterns): first = 1 owns the state
    assert _same_bits(a, _run(dev, c, M, V, ld, state_fill=0x7F))
    # a narrower chunking folds in another order: the same argmax, values within the bound of each other
    b = _run(dev, c, M, V, ld, nc=4096)
    assert torch.equal(a[2], b[2])
    assert float((a[0] - b[0]).abs().max()) <= 2 * REL * float(c["scale"].max() + np.abs(c["lse"]).max())


def test_rejected_calls_write_nothing(dev):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops
    M, V, ld = 3, 70, 72
    z = torch.zeros(M, ld, dtype=torch.bfloat16, device=dev)
    zf = torch.zeros(M, ld + 8, dtype=torch.bfloat16, device=dev)
    targets = torch.full((M,), -1, dtype=torch.int32, device=dev)  # (passes the host's range check for every V tried below)
    state = torch.full((ops.logprob_state_elems(M),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    lse, lp = torch.full((M,), -3.5, device=dev), torch.full((M,), -4.5, device=dev)
    arg = torch.full((M,), -9, dtype=torch.int32, device=dev)
    xw = torch.zeros(M, 8, dtype=torch.bfloat16, device=dev)
    ok = dict(chunk=z, ld=ld, M=M, V=V, col0=0, ncols=ld, targets=targets, state=state, first=True, last=True)

    def call(**kw):
        a = dict(ok, **kw)
        ops.logprob_fold(a["chunk"], a["ld"], a["M"], a["V"], a["col0"], a["ncols"], a["targets"], a["state"], a["first"],
                         a["last"], a.get("lse", lse), a.get("lp", lp), a.get("arg", arg), lm=a.get("lm"))

    bad = [dict(chunk=zf.view(-1)[1:]), dict(ld=ld + 4), dict(ld=ld - 8), dict(V=0), dict(col0=V), dict(col0=-8), dict(ncols=0),
           dict(ncols=ld + 8), dict(M=0), dict(first=False), dict(last=False), dict(col0=64, ncols=8),
           dict(state=state[:ops.logprob_state_elems(M) - 1]), dict(lm=(xw, 4, xw, 8, 1, 8)), dict(lm=(xw, 8, xw, 0, 1, 8)),
           dict(lm=(xw, 8, xw, 8, 1, 0))]
    for kw in bad:
        with pytest.raises(_lib.TmiError):
            call(**kw)
    # a bad dtype and null outputs on the last chunk cannot be said through the wrapper
    h, s = _lib.lib(), torch.cuda.current_stream().cuda_stream
    args = [z.data_ptr(), ld, 1, M, V, 0, ld, targets.data_ptr(), None, 0, None, 0, 0, 0, state.data_ptr(), state.numel() * 8, 1, 1,
            lse.data_ptr(), lp.data_ptr(), arg.data_ptr(), s]
    for i, v in ((2, 7), (18, None), (19, None), (20, None), (8, xw.data_ptr()), (7, None), (14, None), (0, None)):
        a = list(args)
        a[i] = v
        assert h.tmi_logprob_fold(*a) == -1, i
    # misaligned pointers (no tensor has one): targets / lse / logprob / argmax off a 4-byte, x / w off a 2-byte boundary
    lm = {8: xw.data_ptr(), 9: 8, 10: xw.data_ptr(), 11: 8, 12: 1, 13: 8}
    for i, off, extra in ((7, 2, {}), (18, 2, {}), (19, 1, {}), (20, 2, {}), (8, 1, lm), (10, 1, lm)):
        a = list(args)
        for j, v in extra.items():
            a[j] = v
        a[i] = a[i] + off
        assert h.tmi_logprob_fold(*a) == -1, (i, off)
    # targets the library cannot see are caught on the host before the first chunk
    for t in (V, -2):
        with pytest.raises(ValueError):
            call(targets=torch.tensor([0, t, 1], dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert (state == 0x5A5A5A5A5A5A5A5A).all() and (lse == -3.5).all() and (lp == -4.5).all() and (arg == -9).all()
    call(targets=torch.zeros(M, dtype=torch.int32, device=dev))  # and the unmodified call is accepted
    torch.cuda.synchronize()
    assert (arg == 0).all() and (lp < 0).all()


def test_unvalidated_out_of_range_target_is_flagged_not_read(dev):
    """With the host check switched off, a target >= V is in no chunk: NaN, and the other rows are untouched by it."""
    from tethys_speech_amd import ops
    M, V, ld = 3, 70, 72
    z = torch.zeros(M, ld, device=dev)
    targets = torch.tensor([1, 5000000, -1], dtype=torch.int32, device=dev)
    state = torch.empty(ops.logprob_state_elems(M), dtype=torch.int64, device=dev)
    lse, lp, arg = torch.empty(M, device=dev), torch.empty(M, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    ops.logprob_from_logits(z, V, targets, state, lse, lp, arg, validate=False)
    torch.cuda.synchronize()
    assert torch.isnan(lp[1]) and float(lp[2]) == 0.0 and abs(float(lp[0]) + np.log(V)) < 1e-5 and (arg == 0).all()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_recorded_plan_replays_the_direct_call(dev, mode):
    from tethys_speech_amd import ops
    from tethys_speech_amd.plan import LaunchPlan
    M, V, ld = 17, 8192 + 5, 8192 + 8
    c = _case(M, V, ld, mode)
    direct = _run(dev, c, M, V, ld)
    z, targets = c["z"].to(dev), c["targets"].to(dev)
    lm = (c["x"].to(dev), D_LM, c["w"].to(dev), ld, 1, D_LM) if c["x"] is not None else None
    state = torch.empty(ops.logprob_state_elems(M), dtype=torch.int64, device=dev)
    out = [torch.zeros(M, device=dev), torch.zeros(M, device=dev), torch.zeros(M, dtype=torch.int32, device=dev)]
    plan = LaunchPlan()
    with plan.recording():
        ops.logprob_from_logits(z, V, targets, state, *out, lm=lm, validate=False)
    torch.cuda.synchronize()
    assert plan.launches == 2 and _same_bits(direct, [t.cpu() for t in out])
    for t in out:
        t.zero_()
    state.zero_()
    plan.replay()
    torch.cuda.synchronize()
    assert _same_bits(direct, [t.cpu() for t in out])
