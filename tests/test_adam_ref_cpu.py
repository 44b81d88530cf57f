"""tests/_adam_ref.py sets the bounds of tests/test_optimizer_kernels_gpu.py, so it is checked here first, without a GPU:
against the project's oracle, against torch.optim (a source of truth the project did not write), and its analytic fp32
bounds against a plain fp32 restatement of the kernel's arithmetic on the very inputs the GPU tests use."""
import numpy as np
import pytest
import torch

import _adam_ref as R
from oracle import whisper_oracle as O

# exactly representable in fp32, with 1 - beta and 1 - lr * weight_decay exact in fp32 too: the reference's fp32 constants
# and the textbook's doubles are then the same numbers
EXACT = dict(lr=2.0 ** -13, beta1=0.875, beta2=0.9990234375, eps=2.0 ** -23)
EXACT_WD = 0.125   # lr * wd = 2^-16, 1 - 2^-16 fits fp32


def _draw(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g, dtype=torch.float64) * s for s in (1.0, 0.02, 0.02, 0.02)]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_exact_constants_are_exact():
    c = R.adam_constants(step=3, eps_mode=0, weight_decay=EXACT_WD, **EXACT)
    assert c["omb1"] == 1.0 - EXACT["beta1"] and c["omb2"] == 1.0 - EXACT["beta2"]
    assert c["decay"] == 1.0 - EXACT["lr"] * EXACT_WD
    # and the case the reference exists for: fp32 1 - 0.999 is not 0.001
    c = R.adam_constants(step=1, eps_mode=0, **R.HYPER)
    assert c["omb2"] == float(np.float32(1.0) - np.float32(0.999)) and abs(c["omb2"] - 1e-3) > 1e-8


@pytest.mark.parametrize("weight_decay", [0.0, EXACT_WD])
@pytest.mark.parametrize("eps_mode", [0, 1])
def test_against_the_projects_oracle(eps_mode, weight_decay):
    p, g1, g2, g3 = _draw(2000, 5)
    gscale = 0.25   # (a power of two: pre-scaling the oracle's gradient is exact)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    params, st = {"w": p.clone()}, O.AdamState()
    for step, g in enumerate((g1, g2, g3), start=1):
        p, m, v, _ = R.adam_ref(p, g, m, v, step=step, eps_mode=eps_mode, weight_decay=weight_decay, gscale=gscale,
                                fp32_step_scalars=False, **EXACT)
        O.adam_step(params, {"w": g * gscale}, st, eps_mode="tf" if eps_mode == 0 else "torch", weight_decay=weight_decay, **EXACT)
        assert _rel(p, params["w"]) <= 1e-14 and _rel(m, st.m["w"]) <= 1e-14 and _rel(v, st.v["w"]) <= 1e-14, step


@pytest.mark.parametrize("weight_decay", [0.0, EXACT_WD])
def test_against_torch_optim(weight_decay):
    p, g1, g2, g3 = _draw(2000, 6)
    w = torch.nn.Parameter(p.clone())
    kw = dict(lr=EXACT["lr"], betas=(EXACT["beta1"], EXACT["beta2"]), eps=EXACT["eps"])
    opt = torch.optim.AdamW([w], weight_decay=weight_decay, **kw) if weight_decay else torch.optim.Adam([w], **kw)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step, g in enumerate((g1, g2, g3), start=1):
        p, m, v, _ = R.adam_ref(p, g, m, v, step=step, eps_mode=1, weight_decay=weight_decay, fp32_step_scalars=False, **EXACT)
        w.grad = g.clone()
        opt.step()
        s = opt.state[w]
        assert _rel(p, w.detach()) <= 1e-12 and _rel(m, s["exp_avg"]) <= 1e-12 and _rel(v, s["exp_avg_sq"]) <= 1e-12, step


def test_fp32_step_scalars_move_the_update_by_an_fp32_rounding_only():
    p, g, _, _ = _draw(500, 7)
    z = torch.zeros_like(p)
    a = R.adam_terms(p, g, z, z, step=7, eps_mode=1, **R.HYPER)
    b = R.adam_terms(p, g, z, z, step=7, eps_mode=1, fp32_step_scalars=False, **R.HYPER)
    d = float(((a["upd"] - b["upd"]).abs() / b["upd"].abs()).max())
    assert 0.0 < d <= 2 * R.U


@pytest.mark.parametrize("n,eps_mode,weight_decay,gscale,step,zero_grad",
                         [c for c in R.adam_cases() if c[0] in (3, 1027, 4 * 256 * 3 + 2, R.WRAPPED_N)])
def test_restatement_stays_within_the_analytic_bounds(n, eps_mode, weight_decay, gscale, step, zero_grad):
    """The bounds hold for a plain fp32 evaluation: whatever the kernel is later measured at, the bounds were not fitted to it.
    Two consecutive steps as in the GPU test, the second from the restatement's own p, m, v."""
    p, g, g2, m, v = R.adam_inputs(n)
    kw = dict(eps_mode=eps_mode, weight_decay=weight_decay, gscale=gscale, **R.HYPER)
    worst = {}
    for k, grad in enumerate((g, g2)):
        t = R.adam_terms(p, grad, m, v, step=step + k, **kw)
        b = R.adam_bounds(t)
        assert b["k"] == (3, 5, 5 if eps_mode == 0 else 6)
        p, m, v, mirror = R.adam_restate_fp32(p, grad, m, v, step=step + k, **kw)
        for name, got in (("p", p), ("m", m), ("v", v)):
            worst[name] = max(worst.get(name, 0.0), R.bound_fraction(got, t[name], b[name]))
        assert torch.equal(R.bf16_bits(mirror), R.bf16_rne_bits(p))
    assert all(f <= 1.0 for f in worst.values()), worst
    if n >= 1027:   # (a bound a plain evaluation never comes near would say nothing)
        assert all(f >= 0.05 for f in worst.values()), worst


def test_bounds_notice_a_wrong_constant():
    """0.001f in place of 1.0f - b2 moves v by up to 1.3e-5 relative, some forty times the 5 u bound."""
    p, g, _, m, v = R.adam_inputs(1027)
    t = R.adam_terms(p, g, m, v, step=2, eps_mode=0, **R.HYPER)
    b = R.adam_bounds(t)
    wrong = 0.999 * v.double() + 0.001 * g.double() ** 2
    assert R.bound_fraction(wrong, t["v"], b["v"]) > 20.0


def test_planted_inputs_are_what_they_claim():
    p, g, g2, m, v = R.adam_inputs(1027)
    cls = R.element_class(1027)
    bits = p.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    for which, parity in ((R.ZERO_TIE_EVEN, 0), (R.ZERO_TIE_ODD, 1)):
        sel = cls == which
        assert int(sel.sum()) > 30 and torch.all((bits[sel] & 0xFFFF) == 0x8000) and torch.all(((bits[sel] >> 16) & 1) == parity)
        assert float(g[sel].abs().max()) == 0.0 and float(m[sel].abs().max()) == 0.0 and float(v[sel].abs().max()) == 0.0
        # ties go to the even upper half: down when it is even already, up (in magnitude) when it is odd
        want = (bits[sel] >> 16) + parity
        assert torch.equal(R.bf16_rne_bits(p[sel]).to(torch.int64), want)
        assert torch.equal(R.bf16_bits(p[sel].to(torch.bfloat16)).to(torch.int64), want)
        assert bool((p[sel] < 0).any()) and bool((p[sel] > 0).any())
    assert float(v.min()) >= 0.0 and bool((p < 0).any())
    assert torch.all(g[cls == R.G_HUGE].abs() == 1e4) and torch.all(g[cls == R.G_TINY].abs() == np.float32(1e-12))
    assert torch.all(v[cls == R.V_LARGE_M_TINY] == 1e6) and torch.all(m[cls == R.V_LARGE_M_TINY].abs() == np.float32(1e-20))


def test_case_table_covers_every_axis_at_every_length():
    cases = R.adam_cases()
    assert len(cases) == 36
    for n in R.ADAM_NS:
        mine = [c for c in cases if c[0] == n]
        assert {c[1] for c in mine} == {0, 1} and {(c[2], c[3]) for c in mine} == {(0.0, 1.0), (0.1, 0.125)}
        assert {c[4] for c in mine} == {1, 2, 1000} and {c[5] for c in mine} == {False, True}


def test_unpack_ref_and_clip_factors():
    src = torch.arange(24, dtype=torch.float32)
    got = R.unpack_ref(src, 3, 8, 5, 0.5)
    assert torch.equal(got, (src[0:5] + src[8:13] + src[16:21]) * 0.5)
    ss = torch.tensor([4.0, 0.25, 0.0], dtype=torch.float64)
    cg, cs = R.clip_factors(ss, torch.tensor([0, 1, 2, 2]), 1.0, 0.5)
    assert abs(cg - 1.0 / 4.25 ** 0.5) < 1e-15
    want = torch.tensor([0.5 / (cg * 2.0), 1.0, 1.0, 1.0], dtype=torch.float64)   # cg * 0.5 < 0.5: not clipped
    assert float((cs - want).abs().max()) < 1e-15
    cg, cs = R.clip_factors(ss, torch.tensor([0, 1]), 0.0, 0.0)
    assert cg == 1.0 and torch.equal(cs, torch.ones(2, dtype=torch.float64))
