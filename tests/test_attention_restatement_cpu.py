"""The bf16-rounding restatement of attention in tests/test_attention_forms_gpu.py sets that file's bounds (twice its own
error against float64), so it is checked here, without a GPU: its whole-tensor error stays below the 1.5e-2 that
tests/test_kernels_gpu.py::test_flash_attention allows the kernels, and a restatement stripped of its roundings is the
reference itself."""
import pytest
import torch

import _layout_ref as L
import test_attention_forms_gpu as F

BOUND = 1.5e-2  # test_flash_attention's bound for bf16 gradients


def _case(B, H, Tq, Tk, mask, scale, drop, seed, q_std, lag=0.0):
    inp = F.gaussian(B, H, Tq, Tk, seed, q_std=q_std)
    keep, ks = None, 1.0
    if drop > 0:
        from oracle import dropout as DO
        keep, ks = DO.keep_attention(seed, B, H, Tq, Tk, drop), DO.keep_scale(drop)
    rest = F.Errors()
    for b in range(B):
        q, k, v, do = (F.heads(inp[n][b], H) for n in ("q", "k", "v", "do"))
        kp = None if keep is None else torch.from_numpy(keep[b])
        ref = F.reference(q, k, v, do, mask, scale, 0.5, kp, ks)
        rst = F.restate(q, k, v, do, mask, scale, 0.5, kp, ks, lag=lag)
        for name in ref:
            rest.add(name, rst[name], ref[name])
    return rest


@pytest.mark.parametrize("lag", F.LAGS)
@pytest.mark.parametrize("B,H,Tq,Tk,mask,scale,drop,q_std", [(2, 2, 100, 100, 1, 1.0, 0.0, 0.35), (1, 2, 70, 333, 0, 0.125, 0.1, 1.0)])
def test_restatement_stays_close_to_float64(B, H, Tq, Tk, mask, scale, drop, q_std, lag):
    rest = _case(B, H, Tq, Tk, mask, scale, drop, 40 + Tq, q_std, lag)
    for name in ("o", "dq", "dk", "dv"):
        whole = rest.metric(name, "whole")
        assert 0.0 < whole < BOUND, (name, whole)   # (0 would mean the roundings are gone)
        for which in F.METRICS[name]:
            assert rest.metric(name, which) < 4 * BOUND, (name, which, rest.metric(name, which))


def _rate_case(B, H, Tq, Tk, mask, p, mask_seed, lag):
    """_case with the dropout seed apart from the inputs' (tests/_layout_ref.ATTN_RATE_CASES)."""
    from oracle import dropout as DO
    inp = F.gaussian(B, H, Tq, Tk, 1400 + Tk)
    keep, ks = DO.keep_attention(mask_seed, B, H, Tq, Tk, p), DO.keep_scale(p)
    rest = F.Errors()
    for b in range(B):
        q, k, v, do = (F.heads(inp[n][b], H) for n in ("q", "k", "v", "do"))
        kp = torch.from_numpy(keep[b])
        ref = F.reference(q, k, v, do, mask, 1.0, 0.5, kp, ks)
        rst = F.restate(q, k, v, do, mask, 1.0, 0.5, kp, ks, lag=lag)
        for name in ref:
            rest.add(name, rst[name], ref[name])
    return rest


@pytest.mark.parametrize("lag", F.LAGS)
@pytest.mark.parametrize("thr,p", L.RATES, ids=L.RATE_IDS)
def test_restatement_stays_close_to_float64_at_every_dropout_rate(thr, p, lag):
    """The rates of tests/test_dropout_rates_gpu.py on its smallest shape and seed, before a kernel is judged by twice this
    error: from two dropped scores (thr = 1) to ONE kept score of 104000 under a keep scale of 65536 (thr = 65535)."""
    B, H, Tq, Tk, mask, seed = L.ATTN_RATE_CASES[0]
    rest = _rate_case(B, H, Tq, Tk, mask, p, seed, lag)
    for name in ("o", "dq", "dk", "dv"):
        whole = rest.metric(name, "whole")
        assert 0.0 < whole < BOUND, (name, thr, whole)
        for which in F.METRICS[name]:
            assert rest.metric(name, which) < 4 * BOUND, (name, which, thr, rest.metric(name, which))


def test_restatement_without_roundings_is_the_reference(monkeypatch):
    monkeypatch.setattr(F, "bf", lambda t: t)
    rest = _case(1, 2, 130, 130, 1, 0.125, 0.1, 7, 1.0, lag=1.0 / 3.0)
    for name in ("o", "dq", "dk", "dv"):
        assert rest.metric(name, "whole") < 1e-12, (name, rest.metric(name, "whole"))
