"""The Wav2Vec2 evaluation kernels (csrc/score.hip) against float64: ``tmi_contrastive_score`` - the gathered contrastive loss
and its argmax flag with the rule for padded frames - and ``tmi_vq_count``, at the shapes where their loops change path
(one and several 64-item trips per lane, pd below / not a multiple of / above a wave's width, a row stride wider than pd,
both index layouts, a last workgroup that is not full, several workgroups of the histogram).

Inputs and outputs are slices of guard-filled buffers, compared bit for bit after the call (the harness of
tests/test_w2v_kernels_gpu.py).  The reference is tests/_w2v_eval_ref.py on the STORED values (bf16: the inputs are rounded to
bf16 first; the temperature is the fp32 value the call receives).  No bound is fitted to the kernel.  With U = 2^-24:

  a logit:    e_j = (pd + 2) U sum_k |h_k q_jk| / temperature - the pd roundings of the fma chain, the reciprocal of the
              temperature, the product with it;
  a row loss: e_0 + max_n e_n + (Nn + 8) U max(1, |loss_ref|).  The first two terms carry the logit errors through
              logsumexp - logit_0 (a convex combination of the e_n, plus e_0).  The last covers the kernel's own roundings,
              counted for its order (the header comment of the kernel; expf / logf of the device library: 1 ulp).  Relative to
              the sum s >= 1: the rounding of z - m in each exponent, <= U |d| exp(-|d|) <= U / e per term; expf 1; a lane's
              online fold over its trips = ceil((Nn + 1) / 64) items: trips adds and at most trips - 1 rescales of (expf, product,
              exponent) ~ 3.4 each; the lane's one rescale to the row maximum 3.4 (exact for a lane with one item, and for the
              lane that holds the maximum); the butterfly <= 6 adds; logf 1; then (max - logit_0) and the final sum, U |loss| each.
              One trip (Nn <= 63): (Nn + 1) / e + 1 + 6 + 1 + 2 <= Nn + 8.  Several: (Nn + 1)(1 / e + 4.4 / 64) + 17 <= Nn + 8 from
              Nn = 16 on.  So the stated budget holds for this arithmetic as it is.
  the flag:   equal to the reference's wherever |logit_0 - max kept negative| > e_0 + max_n e_n; rows inside that band may go
              either way, and at most 1 % of a case's rows may lie in it (a condition on the inputs, asserted).  A reference gap
              of exactly 0 - a negative equal to t - must come out correct: the kernel forms both logits on one code path.
"""
import numpy as np
import pytest
import torch

import _w2v_eval_ref as E
from _margins import within
from test_w2v_kernels_gpu import Buf, dname, guard_pattern, same

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
TEMP = float(np.float32(0.1))  # the value the entry point receives
TMI_ERR_INVALID = -1


def _mods():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops, wav2vec2
    return ops, _lib, wav2vec2


class Rows:
    """[B][T][pd] at row stride ld inside a buffer of guard values: the pad columns and both ends are guards."""

    def __init__(self, dev, data, ld, dtype, off=8, trail=64):
        B, T, pd = data.shape
        host = guard_pattern(off + B * T * ld + trail, dtype)
        self.mask = torch.zeros(host.shape, dtype=torch.bool)
        self.mask[off:off + B * T * ld].view(B * T, ld)[:, :pd] = True
        host[self.mask] = data.to(dtype).reshape(-1)
        self.host0, self.t, self.off = host.clone(), host.to(dev), off

    @property
    def v(self):
        return self.t[self.off:]

    def unchanged(self):
        return same(self.t, self.host0)


def make_inputs(B, T, pd, Nn, dtype, seed, per_time=False, scale=1.0):
    _, _, w = _mods()
    g = np.random.default_rng(seed)
    h = g.standard_normal((B, T, pd))
    q = 2.5 / np.sqrt(pd) * h + g.standard_normal((B, T, pd))
    h, q = (torch.from_numpy(a * scale).to(dtype) for a in (h, q))  # the stored values
    neg = w.sample_negative_indices(g, T if per_time else B, T, Nn)
    return h, q, neg


def lengths_mask(B, T):
    lens = [(T, max(1, int(round(0.65 * T))), 1)[b % 3] for b in range(B)]
    return (np.arange(T)[None, :] < np.array(lens)[:, None]).astype(np.float32)


def run_score(dev, h, q, neg, mask, dtype, ld=None, per_time=False, twice=True):
    ops, _, _ = _mods()
    B, T, pd = h.shape
    ld = ld or pd
    Nn = neg.shape[1]
    hb, qb = Rows(dev, h, ld, dtype), Rows(dev, q, ld, dtype)
    nb = Buf(dev, neg.size, torch.int32, torch.from_numpy(neg))
    mb = None if mask is None else Buf(dev, B * T, F32, torch.from_numpy(mask))
    outs = []
    for _ in range(2 if twice else 1):
        loss, corr = Buf(dev, B * T, F32), Buf(dev, B * T, torch.int32)
        ops.contrastive_score(hb.v, qb.v, nb.v, loss.v, corr.v, B, T, pd, Nn, TEMP, mask=None if mb is None else mb.v,
                              per_time=per_time, ld=ld)
        torch.cuda.synchronize()
        assert loss.guards_ok() and corr.guards_ok(), "a store outside the outputs"
        outs.append((loss.rows().reshape(B, T), corr.rows().reshape(B, T)))
    assert hb.unchanged() and qb.unchanged() and nb.guards_ok() and same(nb.rows().reshape(-1), torch.from_numpy(neg).reshape(-1))
    assert mb is None or (mb.guards_ok() and same(mb.rows().reshape(-1), torch.from_numpy(mask).reshape(-1)))
    if twice:
        assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1]), "two runs must be bit-identical"
    return outs[0][0].double().numpy(), outs[0][1].numpy()


def judge(name, loss, corr, ref, pd, Nn, band_share=0.01):
    assert np.isfinite(loss).all(), (name, "non-finite loss")
    bound, band = E.bounds(ref, pd, Nn)
    valid = ref["valid"]
    assert (loss[~valid] == 0).all() and (corr[~valid] == 0).all(), (name, "a masked row must give loss 0, correct 0")
    assert (loss >= 0).all(), (name, "a row loss is a -log of a probability")
    err = np.abs(loss - ref["row_loss"])
    frac = float((err / bound).max())
    inside = valid & (np.abs(ref["gap"]) <= band) & (ref["gap"] != 0)
    share = inside.sum() / valid.size
    acc = ref["row_correct"][valid].mean()
    print(f"{name}: loss error {frac:.3f} of its bound (max abs {err.max():.3e}); {int(inside.sum())} of {valid.size} rows in "
          f"the flag band; reference accuracy {acc:.3f}")
    within(f"w2v score {name} row loss / bound", frac, 1.0)
    assert share <= band_share, (name, "too many rows inside the flag band", int(inside.sum()), valid.size)
    decided = valid & ~inside
    assert (corr[decided] == ref["row_correct"][decided]).all(), (name, "flag differs outside the band")
    assert set(np.unique(corr)) <= {0, 1}
    tie = valid & (ref["gap"] == 0)
    assert (corr[tie] == 1).all(), (name, "an exact tie with the positive must count as correct")


# (B, T, pd, Nn, ld, per_time)
SHAPES = [(2, 7, 8, 3, None, False),         # the smallest case
          (1, 100, 256, 100, None, False),   # one workload row: two trips per lane
          (3, 67, 40, 100, 48, False),       # Nn > T - 1: the sampler tiles repeats; pd no multiple of 64; row stride 48; 201 rows
          (2, 130, 128, 130, None, False),   # more than 128 negatives: three trips
          (2, 50, 64, 20, None, True)]       # the [T][Nn] layout
IDS = ["2x7x8x3", "1x100x256x100", "3x67x40x100_ld48", "2x130x128x130", "2x50x64x20_per_time"]


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_contrastive_score_matches_float64(dev, shape, dtype, masked):
    B, T, pd, Nn, ld, per_time = shape
    h, q, neg = make_inputs(B, T, pd, Nn, dtype, seed=B * 1000 + T, per_time=per_time)
    mask = lengths_mask(B, T) if masked else None
    loss, corr = run_score(dev, h, q, neg, mask, dtype, ld=ld, per_time=per_time)
    ref = E.score(h.double().numpy(), q.double().numpy(), neg, TEMP, mask, per_time)
    name = f"{IDS[SHAPES.index(shape)]} {dname(dtype)} {'masked' if masked else 'unmasked'}"
    judge(name, loss, corr, ref, pd, Nn)
    if masked and B >= 3:  # the clip with one valid frame keeps only negatives that name that frame
        assert corr[2, 0] == 1 and (corr[2, 1:] == 0).all()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_contrastive_score_rows_longer_than_one_staged_piece(dev, dtype):
    """pd above the 1024 elements of h_t the kernel stages at a time: two pieces (the second of 8 elements), restaged on
    each of the two trips of a lane, with a mask."""
    B, T, pd, Nn = 2, 5, 1032, 70
    h, q, neg = make_inputs(B, T, pd, Nn, dtype, seed=21, scale=0.125)  # (scaled: logits of a size at which the negatives count)
    mask = lengths_mask(B, T)
    loss, corr = run_score(dev, h, q, neg, mask, dtype)
    ref = E.score(h.double().numpy(), q.double().numpy(), neg, TEMP, mask)
    judge(f"2x5x1032x70 {dname(dtype)} masked", loss, corr, ref, pd, Nn, band_share=1.0)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_contrastive_score_special_rows(dev, dtype):
    # a negative equal to t, with every other frame far below: the two logits tie bit for bit
    B, T, pd, Nn = 2, 9, 24 if dtype == F32 else 16, 5
    h, q, neg = make_inputs(B, T, pd, Nn, dtype, seed=11)
    neg = neg.copy()
    neg[:, 2] = np.arange(B) + 3      # row (b, b + 3) names itself
    loss, corr = run_score(dev, h, q, neg, None, dtype)
    ref = E.score(h.double().numpy(), q.double().numpy(), neg, TEMP)
    assert all(ref["gap"][b, b + 3] <= 0 for b in range(B))
    judge(f"self-negative {dname(dtype)}", loss, corr, ref, pd, Nn, band_share=1.0)
    for b in range(B):
        if ref["gap"][b, b + 3] == 0:
            assert corr[b, b + 3] == 1
    hq = torch.from_numpy(np.random.default_rng(5).standard_normal((1, 6, pd))).to(dtype)
    only_self = np.zeros((1, 4), dtype=np.int32)
    l2, c2 = run_score(dev, hq, hq, only_self, None, dtype)  # row 0: the positive five times
    assert c2[0, 0] == 1 and abs(l2[0, 0] - np.log(5.0)) <= 13 * E.U * np.log(5.0)

    # rows where every negative is masked: loss exactly 0, correct 1; the masked rows 0 / 0
    mask = np.zeros((1, 10), dtype=np.float32)
    mask[0, :4] = 1
    h, q, _ = make_inputs(1, 10, pd, 3, dtype, seed=12)
    loss, corr = run_score(dev, h, q, np.array([[5, 7, 9]], dtype=np.int32), mask, dtype)
    assert (loss == 0).all() and corr[0].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0]

    # a dominant positive, gap > 100: the loss is tiny and never negative
    g = np.random.default_rng(13)
    hd = g.standard_normal((2, 40, 64))
    h, q = torch.from_numpy(hd).to(dtype), torch.from_numpy(3.0 * hd).to(dtype)
    neg = np.stack([g.permutation(40)[:20] for _ in range(2)]).astype(np.int32)
    ref = E.score(h.double().numpy(), q.double().numpy(), neg, TEMP)
    dominant = ref["gap"] > 100  # (a row whose own frame is among its batch row's negatives ties instead: gap 0)
    assert (dominant | (ref["gap"] == 0)).all() and dominant.sum() >= 30
    loss, corr = run_score(dev, h, q, neg, None, dtype)
    judge(f"dominant positive {dname(dtype)}", loss, corr, ref, 64, 20, band_share=1.0)
    assert (loss >= 0).all() and (loss[dominant] < 1e-30).all() and (corr[dominant] == 1).all()

    # inputs scaled by 4: logits in the thousands
    h, q, neg = make_inputs(2, 50, 64, 20, dtype, seed=14, scale=4.0)
    ref = E.score(h.double().numpy(), q.double().numpy(), neg, TEMP)
    assert np.abs(ref["z"]).max() > 1000
    loss, corr = run_score(dev, h, q, neg, None, dtype)
    assert np.isfinite(loss).all()
    judge(f"scaled by 4 {dname(dtype)}", loss, corr, ref, 64, 20, band_share=1.0)


def test_contrastive_score_rejections_write_nothing(dev):
    ops, _lib, _ = _mods()
    lib = _lib.lib()
    B, T, pd, Nn = 2, 7, 8, 3
    h, q, neg = make_inputs(B, T, pd, Nn, F32, seed=1)
    hb, qb = Rows(dev, h, pd, F32), Rows(dev, q, pd, F32)
    nb = Buf(dev, neg.size, torch.int32, torch.from_numpy(neg))
    mb = Buf(dev, B * T, F32, torch.ones(B * T))
    loss, corr = Buf(dev, B * T, F32), Buf(dev, B * T, torch.int32)
    ok = dict(h=hb.v.data_ptr(), q=qb.v.data_ptr(), ld=pd, dtype=0, neg=nb.v.data_ptr(), sb=Nn, st=0, mask=mb.v.data_ptr(),
              loss=loss.v.data_ptr(), corr=corr.v.data_ptr(), B=B, T=T, pd=pd, Nn=Nn, temp=TEMP)

    def call(**kw):
        v = {**ok, **kw}
        return lib.tmi_contrastive_score(v["h"], v["q"], v["ld"], v["dtype"], v["neg"], v["sb"], v["st"], v["mask"], v["loss"],
                                         v["corr"], v["B"], v["T"], v["pd"], v["Nn"], v["temp"], ops.stream())

    for bad in (dict(h=None), dict(q=None), dict(neg=None), dict(loss=None), dict(corr=None), dict(h=ok["h"] + 4),
                dict(q=ok["q"] + 8), dict(pd=6, ld=6), dict(dtype=1, pd=4, ld=4), dict(ld=4), dict(ld=10), dict(B=0), dict(T=0), dict(Nn=0),
                dict(T=(1 << 30) + 1), dict(B=1 << 16, T=1 << 15), dict(temp=0.0), dict(temp=-0.1), dict(dtype=3), dict(st=-1)):
        assert call(**bad) == TMI_ERR_INVALID, bad
        assert b"tmi_contrastive_score" in lib.tmi_last_error()
    torch.cuda.synchronize()
    assert same(loss.t, loss.host0) and same(corr.t, corr.host0), "a rejected call wrote something"
    # index values live on the device: the wrapper checks them on the host before anything is launched
    for v in (-1, T):
        bad_neg = torch.from_numpy(neg).clone()
        bad_neg[1, 1] = v
        with pytest.raises(ValueError):
            ops.contrastive_score(hb.v, qb.v, bad_neg.to(dev), loss.v, corr.v, B, T, pd, Nn, TEMP)
    torch.cuda.synchronize()
    assert same(loss.t, loss.host0) and same(corr.t, corr.host0)
    assert call() == 0  # the accepted form, for contrast
    torch.cuda.synchronize()
    assert loss.guards_ok() and corr.guards_ok() and bool(torch.isfinite(loss.rows()).all())


# ----------------------------------------------------------------------------- tmi_vq_count
@pytest.mark.parametrize("rows,G,Nc,masked", [(1, 1, 1, False), (37, 3, 5, True), (800, 2, 320, False), (5000, 2, 320, True)],
                         ids=["1x1x1", "37x3x5_masked", "800x2x320", "5000x2x320_masked"])
def test_vq_count_equals_bincount(dev, rows, G, Nc, masked):
    ops, _, _ = _mods()
    g = np.random.default_rng(rows)
    idx = g.integers(0, Nc, size=(rows, G)).astype(np.int32)
    if rows > 1:  # out-of-range indices are clamped, as tmi_vq_assign clamps them
        idx[0, 0], idx[1, G - 1], idx[rows - 1, 0] = -5, Nc + 3, 2 ** 31 - 1
    mask = (g.random(rows) < 0.6).astype(np.float32) if masked else None
    if masked:
        mask[0], mask[rows - 1] = 1.0, 0.0
    ib = Buf(dev, rows * G, torch.int32, torch.from_numpy(idx))
    mb = None if mask is None else Buf(dev, rows, F32, torch.from_numpy(mask))
    base = g.integers(0, 1000, size=(G, Nc)).astype(np.int64)
    base[0, 0] = 2 ** 40  # (the adds are 64 bit)
    cb = Buf(dev, G * Nc, torch.int64, torch.from_numpy(base))
    want = E.code_counts(idx, Nc, mask)
    assert want.sum() == G * (rows if mask is None else int(mask.sum()))
    for k in (1, 2):  # two calls onto a non-zero base: the call accumulates
        ops.vq_count(ib.v, None if mb is None else mb.v, cb.v.view(G, Nc), rows, G, Nc)
        torch.cuda.synchronize()
        assert np.array_equal(cb.rows().reshape(G, Nc).numpy(), base + k * want)
    assert cb.guards_ok() and ib.guards_ok() and same(ib.rows().reshape(-1), torch.from_numpy(idx).reshape(-1))
    assert mb is None or mb.guards_ok()
    manual = np.stack([np.bincount(np.clip(idx[:, gi].astype(np.int64), 0, Nc - 1)[slice(None) if mask is None else mask > 0],
                                   minlength=Nc) for gi in range(G)])
    assert np.array_equal(manual, want)


def test_vq_count_rejections_write_nothing(dev):
    ops, _lib, _ = _mods()
    lib = _lib.lib()
    ib = Buf(dev, 10, torch.int32, torch.zeros(10))
    cb = Buf(dev, 6, torch.int64, torch.zeros(6))
    i, c = ib.v.data_ptr(), cb.v.data_ptr()
    for bad in ((None, None, c, 5, 2, 3), (i, None, None, 5, 2, 3), (i, None, c, 0, 2, 3), (i, None, c, 5, 0, 3),
                (i, None, c, 5, 2, 0), (i, None, c + 4, 5, 2, 3), (i, None, c, 5, 2, 8192), (i, i + 2, c, 5, 2, 3)):
        assert lib.tmi_vq_count(*bad, ops.stream()) == TMI_ERR_INVALID, bad
        assert b"tmi_vq_count" in lib.tmi_last_error()
    torch.cuda.synchronize()
    assert same(cb.t, cb.host0)
