"""The weighted cross-entropy kernels (tmi_xent_weights, tmi_xent_weighted, tmi_linear_xent_weighted, tmi_sum_scale_dev:
the loss of W:596-598 with its normaliser kept on the device) against the fp64 closed form of tests/_masked_loss_ref.py.

Shapes are tests/test_kernels_gpu.py::test_xent's: B, S = 3, 10 and its (V, ld) list - the on-chip bf16 kernel at the
step's own width, with whole padding chunks, at its longest row and with a ragged chunk; the generic bf16 kernel
(60001 columns); both through the fp32 kernel as well.  Bounds are that test's too: the arithmetic of a scored row is the
unweighted one with one more multiply in the gradient scale."""
import functools
import math

import numpy as np
import pytest
import torch

import _masked_loss_ref as M
from _margins import within
from oracle import whisper_oracle as O  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu

B, S = 3, 10
SHAPES = [(51865, 51872), (51865, 51904), (53241, 53248), (1003, 1024), (128, 128), (60001, 60008)]
DTYPES = [torch.float32, torch.bfloat16]


def _ops():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops
    return ops


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def make_mask(b, s):
    """One fixed seeded mask: 0/1 entries, the fractional weights 0.5 and 2.0, a zero at t = 0, sample 1 all zero, and
    a nonzero last column (which W:597 slices off)."""
    rng = np.random.default_rng(2024)
    m = (rng.random((b, s)) < 0.6).astype(np.float32)
    m[0, :4] = (0.0, 0.5, 2.0, 1.0)
    m[1] = 0.0
    m[:, -1] = 1.0
    w = m[:, :-1]
    assert (w == 0).any() and (w == 1).any() and (w == 0.5).any() and (w == 2.0).any()
    assert m[0, 0] == 0 and not w[1].any() and m[:, -1].all() and w[0].any()
    return m


def _labels(b, s):
    _, labels = O.create_dummy_pool(seed=4, n_mels=4, seq_len=8, max_target_length=s, num_samples=b)
    return labels


@functools.lru_cache(maxsize=None)
def _case(dtype, V, ld):
    """Seeded logits (rounded to ``dtype``: the reference sees what the kernel sees) and the fp64 reference, computed once."""
    g = torch.Generator().manual_seed(70)
    z = (torch.randn((B * S, V), generator=g, dtype=torch.float64) * 2.0).to(dtype)
    logits = torch.zeros((B * S, ld), dtype=dtype)
    logits[:, :V] = z
    labels, mask = _labels(B, S), make_mask(B, S)
    loss, d = M.weighted_xent(z.double().view(B, S, V), labels, mask)
    return logits, labels, mask, loss, d


def run_weighted(ops, dev, logits, labels, mask, b, s, V, ld, loss_scale=1.0, lm=None):
    """The three launches of the step -> (row_loss, loss, inv_wsum); ``logits`` becomes the gradient in place."""
    lab = torch.as_tensor(labels).to(dev)
    msk = torch.as_tensor(mask, dtype=torch.float32).to(dev)
    row_w = torch.full((b * s,), float("nan"), device=dev)
    inv = torch.full((1,), float("nan"), device=dev)
    row_loss = torch.full((b * s,), float("nan"), device=dev)
    out = torch.full((1,), float("nan"), device=dev)
    ops.xent_weights(msk, b, s, row_w, inv)
    ops.xent_fwd_bwd_weighted(logits, ld, lab, row_w, inv, row_loss, b, s, V, loss_scale, lm=lm)
    ops.sum_scale_dev(row_loss, out, b * s, inv)
    torch.cuda.synchronize()
    return row_loss, out, inv


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,ld", SHAPES)
def test_weighted_xent_matches_the_closed_form(dev, dtype, V, ld):
    ops = _ops()
    logits0, labels, mask, loss_ref, d_ref = _case(dtype, V, ld)
    logits = logits0.to(dev)
    row_loss, out, inv = run_weighted(ops, dev, logits, labels, mask, B, S, V, ld)
    w = M.weights_of(mask)
    assert float(inv) == float(np.float32(1.0) / np.float32(float(w.sum())))
    name = "fp32" if dtype == torch.float32 else "bf16"
    dl = abs(float(out) - loss_ref)
    ge = rel_err(logits[:, :V].reshape(B, S, V), d_ref)
    print(f"weighted xent {name} V={V} ld={ld}: |dloss| {dl:.3e} (loss {loss_ref:.6f}), gradient rel_err {ge:.3e}")
    within(f"weighted xent {name} |dloss| / (1e-5 |loss| + 1e-6)", dl / (1e-5 * abs(loss_ref) + 1e-6), 1.0, (V, ld, float(out), loss_ref))
    within(f"weighted xent {name} gradient rel_err", ge, 1e-5 if dtype == torch.float32 else 8e-3, (V, ld))  # measured 5.8e-8 / 1.7e-3
    if ld > V:
        assert float(logits[:, V:].abs().max()) == 0.0
    # unscored rows: exact zeros over all ld columns, row_loss 0
    dead = (w.reshape(-1) == 0).to(dev)
    assert int(dead.sum()) > B and float(logits[dead].abs().max()) == 0.0 and float(row_loss[dead].abs().max()) == 0.0
    assert not torch.signbit(logits[dead].float()).any()
    assert bool((row_loss[~dead] > 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,ld", SHAPES)
def test_all_ones_mask_is_bit_identical_to_the_unmasked_entry(dev, dtype, V, ld):
    ops = _ops()
    logits0, labels, _, _, _ = _case(dtype, V, ld)
    plain, weighted = logits0.to(dev), logits0.to(dev)
    lab = torch.from_numpy(labels).to(dev)
    rl_plain, out_plain = torch.empty(B * S, device=dev), torch.empty(1, device=dev)
    gs = 1.0 / (B * (S - 1))
    ops.xent_fwd_bwd(plain, ld, lab, rl_plain, B, S, V, gs)
    ops.sum_scale(rl_plain, out_plain, B * S, gs)
    rl, out, _ = run_weighted(ops, dev, weighted, labels, np.ones((B, S), dtype=np.float32), B, S, V, ld)
    assert torch.equal(rl, rl_plain) and torch.equal(out, out_plain) and torch.equal(weighted, plain)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,ld", [(51865, 51904), (1003, 1024), (60001, 60008)])
def test_unscored_rows_are_never_read(dev, dtype, V, ld):
    """NaN and Inf in every unscored row: exact zeros come out, and the loss is the loss with those rows finite."""
    ops = _ops()
    logits0, labels, mask, _, _ = _case(dtype, V, ld)
    clean = logits0.to(dev)
    rl0, out0, _ = run_weighted(ops, dev, clean, labels, mask, B, S, V, ld)
    dead = (M.weights_of(mask).reshape(-1) == 0).to(dev)
    dirty = logits0.to(dev)
    rows = torch.nonzero(dead).flatten()
    dirty[rows[0::2]] = float("nan")
    dirty[rows[1::2]] = float("inf")
    dirty[rows[1], 1::2] = float("-inf")
    rl, out, _ = run_weighted(ops, dev, dirty, labels, mask, B, S, V, ld)
    assert math.isfinite(float(out)) and torch.equal(out, out0) and torch.equal(rl, rl0)
    assert float(dirty[dead].abs().max()) == 0.0 and float(rl[dead].abs().max()) == 0.0
    assert torch.equal(dirty, clean)  # two runs of the scored rows: bit-identical


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,ld", [(51865, 51904), (60001, 60008)])
def test_all_zero_mask_gives_zero_loss_and_zero_gradients(dev, dtype, V, ld):
    ops = _ops()
    logits0, labels, _, _, _ = _case(dtype, V, ld)
    logits = logits0.to(dev)
    zero = np.zeros((B, S), dtype=np.float32)
    zero[:, -1] = 1.0  # (only the ignored column; negative entries and NaN count as 0 as well)
    zero[0, 0], zero[0, 1] = -1.0, float("nan")
    rl, out, inv = run_weighted(ops, dev, logits, labels, zero, B, S, V, ld)
    assert float(inv) == 0.0 and float(out) == 0.0 and float(rl.abs().max()) == 0.0 and float(logits.abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_runs_are_bit_identical_and_loss_scale_multiplies_the_gradient(dev, dtype):
    ops = _ops()
    V, ld = 51865, 51904
    logits0, labels, mask, _, _ = _case(dtype, V, ld)
    a, b, c = logits0.to(dev), logits0.to(dev), logits0.to(dev)
    ra, oa, ia = run_weighted(ops, dev, a, labels, mask, B, S, V, ld)
    rb, ob, ib = run_weighted(ops, dev, b, labels, mask, B, S, V, ld)
    assert torch.equal(a, b) and torch.equal(ra, rb) and torch.equal(oa, ob) and torch.equal(ia, ib)
    rc, oc, _ = run_weighted(ops, dev, c, labels, mask, B, S, V, ld, loss_scale=0.25)  # (a power of two: exact)
    assert torch.equal(rc, ra) and torch.equal(oc, oa)
    assert torch.equal(c.float(), a.float() * 0.25)


@pytest.mark.parametrize("R_S,d,V,ld", [((3, 10), 96, 1003, 1024), ((2, 7), 768, 51865, 51904), ((2, 5), 64, 60001, 60008)])
def test_weighted_linear_xent_takes_the_target_logit_from_the_operands(dev, R_S, d, V, ld):
    """tmi_linear_xent_weighted on test_linear_xent_takes_the_target_logit_from_the_operands' shapes: the row loss is the
    weight times that test's definition (the target's term at the fp32-recomputed logit, bound 5e-5 as there), the gradient
    is the plain weighted entry's bit for bit, and an all-ones mask reproduces tmi_linear_xent bit for bit."""
    ops = _ops()
    b, s = R_S
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(91)
    x = torch.randn((b * s, d), generator=g, dtype=torch.float64).to(bf).to(dev)
    w = torch.zeros((d, ld), dtype=bf, device=dev)
    w[:, :V] = (torch.randn((d, V), generator=g, dtype=torch.float64) * (2.0 / math.sqrt(d))).to(bf).to(dev)
    labels, mask = _labels(b, s), make_mask(b, s)
    stored = torch.empty((b * s, ld), dtype=bf, device=dev)
    ops.gemm(x, w, stored, b * s, ld, d, d, 1, ld, 1, ld)
    lm = (x, d, w, ld, 1, d)
    plain, lin = stored.clone(), stored.clone()
    rl_plain, _, _ = run_weighted(ops, dev, plain, labels, mask, b, s, V, ld)
    rl, out, inv = run_weighted(ops, dev, lin, labels, mask, b, s, V, ld, lm=lm)
    assert torch.equal(lin, plain)
    z = stored.double()[:, :V].view(b, s, V).cpu()
    z_exact = (x.double() @ w.double())[:, :V].view(b, s, V).cpu()
    tgt = torch.from_numpy(labels)[:, 1:].long()
    zt = z_exact[:, :-1].gather(-1, tgt.unsqueeze(-1)).squeeze(-1)
    zmix = z[:, :-1].clone()
    zmix.scatter_(-1, tgt.unsqueeze(-1), zt.unsqueeze(-1))
    wgt = M.weights_of(mask)[:, :-1]
    want = wgt * (torch.logsumexp(zmix, dim=-1) - zt)
    got = rl.view(b, s).double().cpu()
    assert float(got[:, -1].abs().max()) == 0.0
    within("weighted linear xent row loss |err| / weight", float(((got[:, :-1] - want).abs() / wgt.clamp(min=1.0)).max()), 5e-5, R_S)
    assert abs(float(out) - float(want.sum() / wgt.sum())) <= 1e-5 * float(want.sum() / wgt.sum()) + 1e-6
    # all ones: the unweighted operand-taking entry, bit for bit
    a, c = stored.clone(), stored.clone()
    lab = torch.from_numpy(labels).to(dev)
    rl_a, out_a = torch.empty(b * s, device=dev), torch.empty(1, device=dev)
    gs = 1.0 / (b * (s - 1))
    ops.xent_fwd_bwd(a, ld, lab, rl_a, b, s, V, gs, lm=lm)
    ops.sum_scale(rl_a, out_a, b * s, gs)
    rl_c, out_c, _ = run_weighted(ops, dev, c, labels, np.ones((b, s), dtype=np.float32), b, s, V, ld, lm=lm)
    assert torch.equal(c, a) and torch.equal(rl_c, rl_a) and torch.equal(out_c, out_a)


@pytest.mark.parametrize("dtype", DTYPES)
def test_recorded_weighted_calls_replay_the_calls_that_were_made(dev, dtype):
    """The three launches recorded in a plan and replayed on restored inputs give the direct call's bits - and a replay
    follows the mask in its (static) buffer: nothing of it was baked into the plan."""
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops, plan
    V, ld = 1003, 1024
    logits0, labels, mask, _, _ = _case(dtype, V, ld)
    direct = logits0.to(dev)
    rl_d, out_d, _ = run_weighted(ops, dev, direct, labels, mask, B, S, V, ld)
    other = np.ones((B, S), dtype=np.float32)
    direct2 = logits0.to(dev)
    rl_d2, out_d2, _ = run_weighted(ops, dev, direct2, labels, other, B, S, V, ld)
    assert not torch.equal(out_d, out_d2)

    lab, msk, logits = torch.from_numpy(labels).to(dev), torch.from_numpy(mask).to(dev), logits0.to(dev)
    row_w, inv, rl, out = (torch.zeros(n, device=dev) for n in (B * S, 1, B * S, 1))
    p = plan.LaunchPlan()
    with p.recording():
        before = p.launches
        ops.xent_weights(msk, B, S, row_w, inv)
        ops.xent_fwd_bwd_weighted(logits, ld, lab, row_w, inv, rl, B, S, V, 1.0)
        ops.sum_scale_dev(rl, out, B * S, inv)
        assert p.launches == before + 3
    torch.cuda.synchronize()
    assert torch.equal(logits, direct) and torch.equal(rl, rl_d) and torch.equal(out, out_d)
    for m_np, want in ((mask, (direct, rl_d, out_d)), (other, (direct2, rl_d2, out_d2))):
        logits.copy_(logits0.to(dev))
        msk.copy_(torch.from_numpy(m_np).to(dev))
        for t in (row_w, inv, rl, out):
            t.fill_(float("nan"))
        p.replay(0, 0)
        torch.cuda.synchronize()
        assert torch.equal(logits, want[0]) and torch.equal(rl, want[1]) and torch.equal(out, want[2])
