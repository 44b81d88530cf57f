"""tmi_decode_constraints and the constrained LM heads (tmi_lm_head_argmax_c / _topk_c / _sample_c) on the GPU against
tests/_constrain_ref.py.  Inputs, seeds and expected results are built on the host by the reference;
tests/test_constrain_cpu.py shows from the reference alone that every listed mutation changes one of these expectations
and that the undecided rows stay under the 5 % cap."""
import itertools

import numpy as np
import pytest
import torch

import _constrain_ref as R
import _sample_ref as S
from _margins import within

pytestmark = pytest.mark.gpu

GARBAGE = 0x7BADBEEF
REL = S.REL


def _mods():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops
    return ops, _lib


def _bits(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ----------------------------------------------------------------------------- 1. the set builder, exact
@pytest.mark.parametrize("V", R.SET_VS)
def test_decode_constraints_equals_reference(dev, V):
    """M in {1, 5, 17} x t in {1, 2, ngram - 1, ngram, 40, 448} x ngram in {0, 1, 2, 3, 5}, inputs as
    _constrain_ref.set_case describes them: ids -1, V and 2^31 - 1 in the prefix, tokens past t that would change the
    answer, outputs pre-filled with garbage, every other case with two spare words per row that must survive, the
    static words with their bits at or above V set.  Two calls give equal bits."""
    ops, _ = _mods()
    W = R.words(V)
    n = 0
    for c in R.set_cases(V):
        M, t, ld, bl = c["M"], c["t"], c["ld"], c["bits_ld"]
        prefix = torch.from_numpy(c["prefix"]).to(dev)
        static = R.set_case_static(c)
        static_d = _bits(static, dev) if static is not None else None
        exp_seen, exp_banned = R.set_case_expected(c)
        outs = []
        for fill in (GARBAGE, 0x11111111):
            seen = torch.full((M, bl), fill, dtype=torch.int32, device=dev)
            banned = torch.full((M, bl), fill, dtype=torch.int32, device=dev)
            ops.decode_constraints(prefix, ld, M, t, V, seen, banned, ngram=c["ngram"], static_banned=static_d)
            outs.append((_u32(seen), _u32(banned)))
            name = (M, V, t, c["ngram"])
            assert np.array_equal(outs[-1][0][:, :W], exp_seen), ("seen", name)
            assert np.array_equal(outs[-1][1][:, :W], exp_banned), ("banned", name)
            assert (outs[-1][0][:, W:] == fill).all() and (outs[-1][1][:, W:] == fill).all(), ("words past W", name)
        assert np.array_equal(outs[0][0][:, :W], outs[1][0][:, :W]) and np.array_equal(outs[0][1][:, :W], outs[1][1][:, :W])
        n += 1
    assert n == len(R.SET_MS) * sum(len(R.set_ts(g)) for g in R.SET_NGRAMS)


def test_decode_constraints_refusals(dev):
    ops, _lib = _mods()
    h = _lib.lib()
    V, M, t, ld = 160, 3, 4, 8
    W = R.words(V)
    prefix = torch.zeros(M, ld, dtype=torch.int32, device=dev)
    seen = torch.full((M, W), GARBAGE, dtype=torch.int32, device=dev)
    banned = seen.clone()
    ok = dict(prefix=prefix.data_ptr(), ld=ld, M=M, t=t, V=V, static=None, ngram=2, seen=seen.data_ptr(),
              banned=banned.data_ptr(), bits_ld=W)
    bad = [dict(prefix=None), dict(seen=None), dict(banned=None), dict(M=0), dict(M=65536), dict(V=0), dict(V=65537),
           dict(t=0), dict(t=ld + 1), dict(t=65537, ld=70000), dict(ngram=-1), dict(bits_ld=W - 1)]
    for change in bad:
        a = dict(ok, **change)
        rc = h.tmi_decode_constraints(a["prefix"], a["ld"], a["M"], a["t"], a["V"], a["static"], a["ngram"], a["seen"],
                                      a["banned"], a["bits_ld"], ops.stream())
        assert rc == -1, (change, rc)  # TMI_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((seen == GARBAGE).all()) and bool((banned == GARBAGE).all()), "a refused call wrote its outputs"
    # the limits themselves pass: V = 65536, and a prefix of 2^16 tokens
    Vb = 65536
    big = torch.full((1, 65536), 7, dtype=torch.int32, device=dev)
    big[0, -1] = Vb - 1
    s2 = torch.full((1, R.words(Vb)), GARBAGE, dtype=torch.int32, device=dev)
    b2 = s2.clone()
    ops.decode_constraints(big, 65536, 1, 65536, Vb, s2, b2, ngram=2)
    assert np.array_equal(_u32(s2)[0], R.bitset([7, Vb - 1], Vb))
    assert np.array_equal(_u32(b2)[0], R.bitset([], Vb))  # (the last token occurs once: nothing follows it)
    ops.decode_constraints(big, 65536, 1, 65535, Vb, s2, b2, ngram=2)
    assert np.array_equal(_u32(s2)[0], R.bitset([7], Vb)) and np.array_equal(_u32(b2)[0], R.bitset([7], Vb))


# ----------------------------------------------------------------------------- 2. the heads
def _argmax(ops, x, x_ld, w, w_ld, M, d, V, ws=None, cons=None, eos_id=-1, gamma=None, beta=None):
    dev = w.device
    ids = torch.full((M,), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    fresh = ws is None
    ws = torch.zeros(M + 1, dtype=torch.int64, device=dev) if fresh else ws
    if cons is None:
        ops.lm_head_argmax(x, x_ld, w, w_ld, M, d, V, ids, 1, ws, gamma=gamma, beta=beta, eos_id=eos_id, eos_count=cnt)
    else:
        ops.lm_head_argmax_c(x, x_ld, w, w_ld, M, d, V, ids, 1, ws, gamma=gamma, beta=beta, eos_id=eos_id, eos_count=cnt,
                             **cons)
    if fresh:
        torch.cuda.synchronize()
        assert int(ws.abs().sum()) == 0, "the workspace is not left zero"
    return ids, cnt


def _topk(ops, x, x_ld, w, w_ld, M, d, V, N, T=1.0, ws=None, cons=None, gamma=None, beta=None):
    dev = w.device
    ids = torch.full((M, N), -7, dtype=torch.int32, device=dev)
    lp = torch.full((M, N), float("nan"), device=dev)
    lse = torch.full((M,), float("nan"), device=dev)
    fresh = ws is None
    ws = torch.zeros(ops.lm_head_topk_workspace_elems(M, V, N), dtype=torch.int64, device=dev) if fresh else ws
    if cons is None:
        ops.lm_head_topk(x, x_ld, w, w_ld, M, d, V, N, ids, lp, ws, gamma=gamma, beta=beta, temperature=T, lse=lse)
    else:
        ops.lm_head_topk_c(x, x_ld, w, w_ld, M, d, V, N, ids, lp, ws, gamma=gamma, beta=beta, temperature=T, lse=lse, **cons)
    if fresh:
        torch.cuda.synchronize()
        assert int(ws.abs().sum()) == 0, "the workspace is not left zero"
    return ids, lp, lse


def _sample(ops, x, x_ld, w, w_ld, M, d, V, top_k, top_p, T, seed, ws=None, cons=None, finished=None, suppress_id=-1,
            eos_id=-1, pad_id=0, gamma=None, beta=None):
    dev = w.device
    ids = torch.full((M,), -7, dtype=torch.int32, device=dev)
    lp = torch.full((M,), float("nan"), device=dev)
    fin = torch.zeros(M, dtype=torch.int32, device=dev) if finished is None else torch.from_numpy(finished.copy()).to(dev)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    fresh = ws is None
    ws = torch.zeros(ops.lm_head_sample_workspace_elems(M, V, top_k), dtype=torch.int64, device=dev) if fresh else ws
    kw = dict(temperature=T, top_k=top_k, top_p=top_p, seed=seed, suppress_id=suppress_id, eos_id=eos_id, pad_id=pad_id,
              logprob=lp, gamma=gamma, beta=beta)
    if cons is None:
        ops.lm_head_sample(x, x_ld, w, w_ld, M, d, V, ids, 1, fin, cnt, ws, **kw)
    else:
        ops.lm_head_sample_c(x, x_ld, w, w_ld, M, d, V, ids, 1, fin, cnt, ws, **kw, **cons)
    if fresh:
        torch.cuda.synchronize()
        assert int(ws.abs().sum()) == 0, "the workspace is not left zero"
    return ids, lp, fin, cnt


def _np(t, dtype=np.float64):
    return t.cpu().numpy().astype(dtype)


def _check_lp(lp, ref, bound, name):
    """-inf and 0 exactly where the reference has them, never NaN, within ``bound`` elsewhere; -> the worst ratio."""
    assert not np.isnan(lp).any(), (name, "NaN")
    inf = np.isneginf(ref)
    assert np.array_equal(np.isneginf(lp), inf), (name, "-inf")
    with np.errstate(invalid="ignore"):
        err = np.where(inf, 0.0, np.abs(lp - ref))
    return float((err / bound).max())


@pytest.mark.parametrize("d,V", list(itertools.product(R.HEAD_DS, R.HEAD_VS)))
def test_constrained_heads_exact_scores(dev, d, V):
    """Small-integer activations and weights, penalties 2 and 1/2, temperatures 1/2, 1, 2: z' and s are exact, so every
    token is the reference's (the draws within P_TOL of an edge of the running sums excepted: they stay among the
    reference's candidates, and tests/test_constrain_cpu.py caps them) and the log-probabilities differ by the fp32
    logsumexp alone: REL * (scale + |lse|), tests/_sample_ref.py's bound.  Rows by pattern (head_case): the winner
    banned with the runner-up in another workgroup, the winner seen at z > 0, z < 0 and z == 0, seen and banned, all
    but one column banned, every column banned, random sets; pad-position bits set everywhere; finished rows and
    suppress_id in sampling."""
    ops, _ = _mods()
    worst, undecided, total = 0.0, 0, 0
    for M, wdt, penalty in itertools.product(R.HEAD_MS, (torch.bfloat16, torch.float32), R.HEAD_PENALTIES):
        c = R.head_case(d, V, M)
        e = R.head_expected(d, V, M, penalty)
        VP = c["VP"]
        x, w = torch.from_numpy(c["x"]).to(dev).to(wdt), torch.from_numpy(c["w"]).to(dev).to(wdt)
        seen, banned = _bits(c["seen"], dev), _bits(c["banned"], dev)
        cons = dict(seen=seen, banned=banned, penalty=penalty)
        name = f"d{d} V{V} M{M} {wdt} p{penalty}"
        all_banned = ~np.isfinite(e["zp"]).any(axis=1)
        # argmax
        tok, _ = e["argmax"]
        ids, cnt = _argmax(ops, x, d, w, VP, M, d, V, cons=cons, eos_id=int(tok[0]))
        ids = _np(ids, np.int64)
        assert np.array_equal(ids, tok), (name, "argmax", ids, tok)
        assert (ids[all_banned] == 0).all() and int(cnt) == int((tok == tok[0]).sum())
        # top-k
        rid, rlp, rlse, _ = e["topk"]
        kid, klp, klse = _topk(ops, x, d, w, VP, M, d, V, R.HEAD_TOPK_N, cons=cons)
        assert np.array_equal(_np(kid, np.int64), rid), (name, "topk ids")
        bound = REL * (c["scale"] + np.abs(np.where(np.isfinite(rlse), rlse, 0.0)))
        worst = max(worst, _check_lp(_np(klp), rlp, bound[:, None], name), _check_lp(_np(klse), rlse, bound, name))
        assert (_np(kid, np.int64)[all_banned] == np.arange(R.HEAD_TOPK_N)).all() and np.isneginf(_np(klse)[all_banned]).all()
        # sampling
        for (top_k, top_p, T), (stok, slp, dec, allowed) in e["sample"].items():
            dead = (c["finished"] != 0) | ~np.isfinite(np.delete(e["zp"], R.HEAD_SUPPRESS, axis=1)).any(axis=1)
            eos = int(stok[~dead][0]) if (~dead).any() else -1  # (a token some live row draws)
            sid, lp, fin, nfin = _sample(ops, x, d, w, VP, M, d, V, top_k, top_p, T, R.head_seed(d, V, M, penalty, top_k),
                                         cons=cons, finished=c["finished"], suppress_id=R.HEAD_SUPPRESS, eos_id=eos,
                                         pad_id=R.HEAD_PAD)
            sid, lp, fin = _np(sid, np.int64), _np(lp), _np(fin, np.int64)
            assert np.array_equal(sid[dec], stok[dec]), (name, top_k, top_p, T, sid, stok)
            for r in np.nonzero(~dec)[0]:
                assert sid[r] in allowed[r], (name, top_k, r)
            assert (sid[dead] == R.HEAD_PAD).all() and (lp[dead] == 0.0).all(), (name, "finished / nothing to draw")
            live = ~dead
            sp = e["zp"] / T
            sp[:, R.HEAD_SUPPRESS] = -np.inf
            lse = R.lse_rows(sp)
            ref_lp = np.where(live, sp[np.arange(M), np.where(live, sid, 0)] - np.where(live, lse, 0.0), 0.0)
            assert np.isfinite(ref_lp).all(), (name, "a banned or suppressed column was drawn")
            b2 = REL * (c["scale"] / T + np.abs(np.where(live, lse, 0.0)))
            worst = max(worst, float((np.abs(lp - ref_lp) / b2).max()))
            exp_fin = (c["finished"] != 0) | (sid == eos)  # (a row that writes pad_id == eos_id would count too)
            assert np.array_equal(fin != 0, exp_fin) and int(nfin) == int(exp_fin.sum()), (name, "finished")
            undecided += int((~dec).sum())
            total += M
    assert undecided <= R.CAP * total, (undecided, total)
    within(f"lm_head_*_c exact d{d} V{V} |lp - lp64| / (REL (scale + |lse|))", worst, 1.0)


@pytest.mark.parametrize("case", R.RANDOM_CASES, ids=lambda c: f"{c[0]}-d{c[1]}-V{c[2]}-M{c[3]}")
def test_constrained_heads_random_inputs_with_layernorm(dev, case):
    """Random activations through the LayerNorm prologue, random sets, penalty 1.3, temperature 0.7; the last case is the
    real grid (V = 51865, d = 768, M = 16).  Decided rows match token for token; the others stay within the derived
    bound b' (tests/_constrain_ref.py's docstring): the chosen z' within 2 b' of the best, the top-k values and
    log-probabilities within 2 b' of the reference's (b' for s', b' for the logsumexp)."""
    ops, _ = _mods()
    wdt, d, V, M, _ = case
    c, e = R.random_case(*case), R.random_expected(case)
    assert R.cap_ok(e["argmax"][1]) and R.cap_ok(e["topk"][3]) and all(R.cap_ok(v[2]) for v in e["sample"].values())
    VP = c["VP"]
    w, gamma, beta = c["w"].to(dev), c["gamma"].to(dev), c["beta"].to(dev)
    x = c["x"].to(dev)[2:]
    cons = dict(seen=_bits(c["seen"], dev), banned=_bits(c["banned"], dev), penalty=R.RANDOM_PENALTY)
    kw = dict(gamma=gamma, beta=beta)
    ar = np.arange(M)
    # argmax
    tok, dec, b = e["argmax"]
    ids = _np(_argmax(ops, x, 3 * d, w, VP, M, d, V, cons=cons, **kw)[0], np.int64)
    assert np.array_equal(ids[dec], tok[dec]), (ids, tok, dec)
    within(f"lm_head_argmax_c {case[:4]} (max z' - chosen z') / 2 b'", float(((e["zp"].max(1) - e["zp"][ar, ids]) / (2 * b)).max()), 1.0)
    # top-k
    rid, rlp, rlse, dec = e["topk"]
    kid, klp, klse = _topk(ops, x, 3 * d, w, VP, M, d, V, R.RANDOM_N, T=R.RANDOM_T, cons=cons, **kw)
    kid = _np(kid, np.int64)
    assert np.array_equal(kid[dec], rid[dec]), (kid, rid, dec)
    b = e["b"]
    within(f"lm_head_topk_c {case[:4]} |lse - lse64| / b'", _check_lp(_np(klse), rlse, b, case), 1.0)
    within(f"lm_head_topk_c {case[:4]} |lp - lp64| / 2 b'", _check_lp(_np(klp), rlp, 2 * b[:, None], case), 1.0)
    assert not np.isneginf(e["sp"][ar[:, None], kid]).any(), "a banned column among the candidates"
    # sampling
    for (top_k, top_p), (stok, _, dec, allowed) in e["sample"].items():
        sid, lp, _, _ = _sample(ops, x, 3 * d, w, VP, M, d, V, top_k, top_p, R.RANDOM_T, 77 * d + M + 31 * top_k, cons=cons, **kw)
        sid, lp = _np(sid, np.int64), _np(lp)
        assert np.array_equal(sid[dec], stok[dec]), (top_k, top_p, sid, stok, dec)
        for r in np.nonzero(~dec)[0]:
            assert sid[r] in allowed[r], (top_k, r)
        ref_lp = e["sp"][ar, sid] - e["lse"]
        assert np.isfinite(ref_lp).all(), "a banned column was drawn"
        within(f"lm_head_sample_c {case[:4]} |lp - lp64| / 2 b'", float((np.abs(lp - ref_lp) / (2 * b)).max()), 1.0)


def test_empty_constraints_are_the_originals_bit_for_bit(dev):
    """seen = banned = NULL with penalty 1 (the originals' own instantiation) and zero-filled sets with penalty 1 (the
    constrained one) against the original entry points on the same inputs: ids, log-probabilities and lse bit-equal."""
    ops, _ = _mods()
    case = R.RANDOM_CASES[0]
    _, d, V, M, _ = case
    c = R.random_case(*case)
    VP, w, x = c["VP"], c["w"].to(dev), c["x"].to(dev)[2:]
    kw = dict(gamma=c["gamma"].to(dev), beta=c["beta"].to(dev))
    zero = torch.zeros(M, R.words(V), dtype=torch.int32, device=dev)
    for cons in (dict(seen=None, banned=None, penalty=1.0), dict(seen=zero, banned=zero, penalty=1.0),
                 dict(seen=zero, banned=None, penalty=1.0), dict(seen=None, banned=zero, penalty=1.7)):
        a, b = _argmax(ops, x, 3 * d, w, VP, M, d, V, eos_id=3, **kw), _argmax(ops, x, 3 * d, w, VP, M, d, V, cons=cons, eos_id=3, **kw)
        assert all(torch.equal(p, q) for p, q in zip(a, b)), "argmax"
        a = _topk(ops, x, 3 * d, w, VP, M, d, V, 6, T=0.7, **kw)
        b = _topk(ops, x, 3 * d, w, VP, M, d, V, 6, T=0.7, cons=cons, **kw)
        assert all(torch.equal(p, q) for p, q in zip(a, b)), "topk"
        for top_k, top_p in ((8, 0.9), (0, 1.0)):
            a = _sample(ops, x, 3 * d, w, VP, M, d, V, top_k, top_p, 0.7, 5, suppress_id=4, eos_id=2, **kw)
            b = _sample(ops, x, 3 * d, w, VP, M, d, V, top_k, top_p, 0.7, 5, suppress_id=4, eos_id=2, cons=cons, **kw)
            assert all(torch.equal(p, q) for p, q in zip(a, b)), ("sample", top_k)


def test_original_and_constrained_calls_share_a_workspace(dev):
    """Alternating original and _c calls on ONE workspace, no synchronisation in between, give what fresh workspaces give."""
    ops, _ = _mods()
    d, V, M = 64, 1000, 17
    c = R.head_case(d, V, M)
    VP = c["VP"]
    x, w = torch.from_numpy(c["x"]).to(dev), torch.from_numpy(c["w"]).to(dev)
    cons = dict(seen=_bits(c["seen"], dev), banned=_bits(c["banned"], dev), penalty=2.0)
    order = (None, cons, None, cons, cons, None)
    ws = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    got = [_argmax(ops, x, d, w, VP, M, d, V, ws=ws, cons=k) for k in order]
    torch.cuda.synchronize()
    assert int(ws.abs().sum()) == 0
    for k, g in zip(order, got):
        assert torch.equal(g[0], _argmax(ops, x, d, w, VP, M, d, V, cons=k)[0])
    ws = torch.zeros(ops.lm_head_topk_workspace_elems(M, V, 6), dtype=torch.int64, device=dev)
    got = [_topk(ops, x, d, w, VP, M, d, V, 6, ws=ws, cons=k) for k in order]
    torch.cuda.synchronize()
    assert int(ws.abs().sum()) == 0
    for k, g in zip(order, got):
        f = _topk(ops, x, d, w, VP, M, d, V, 6, cons=k)
        assert torch.equal(g[0], f[0]) and torch.equal(g[1], f[1]) and torch.equal(g[2], f[2])
    ws = torch.zeros(ops.lm_head_sample_workspace_elems(M, V, 8), dtype=torch.int64, device=dev)
    got = [_sample(ops, x, d, w, VP, M, d, V, 8, 0.9, 1.0, 3, ws=ws, cons=k, pad_id=3) for k in order]
    torch.cuda.synchronize()
    assert int(ws.abs().sum()) == 0
    for k, g in zip(order, got):
        f = _sample(ops, x, d, w, VP, M, d, V, 8, 0.9, 1.0, 3, cons=k, pad_id=3)
        assert torch.equal(g[0], f[0]) and torch.equal(g[1], f[1])


def test_constrained_heads_refusals(dev):
    """A bad constraint argument is TMI_ERR_INVALID on every _c entry point and writes nothing; the originals' own
    refusals are shared code (one bad size here)."""
    ops, _lib = _mods()
    from tethys_speech_amd._lib import TmiError
    d, V, M = 64, 130, 3
    c = R.head_case(d, V, M)
    VP, W = c["VP"], R.words(V)
    x, w = torch.from_numpy(c["x"]).to(dev), torch.from_numpy(c["w"]).to(dev)
    seen, banned = _bits(c["seen"], dev), _bits(c["banned"], dev)
    h = _lib.lib()
    ids = torch.full((M,), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ws = torch.zeros(64, dtype=torch.int64, device=dev)

    def argmax_rc(seen_p, banned_p, bits_ld, penalty, Vv=V):
        return h.tmi_lm_head_argmax_c(x.data_ptr(), d, 0, None, None, 1e-5, w.data_ptr(), VP, 0, M, d, Vv, ids.data_ptr(), 1, -1,
                                      cnt.data_ptr(), ws.data_ptr(), 8 * ws.numel(), seen_p, banned_p, bits_ld, penalty,
                                      ops.stream())

    sp, bp = seen.data_ptr(), banned.data_ptr()
    assert argmax_rc(sp, bp, W + 1, 2.0) == 0
    torch.cuda.synchronize()
    ids.fill_(-7)
    for args in ((sp, bp, W - 1, 2.0), (sp, None, W - 1, 2.0), (sp, bp, W + 1, 0.0), (sp, bp, W + 1, -1.0),
                 (sp, bp, W + 1, float("inf")), (sp, bp, W + 1, float("nan")), (None, None, 0, 0.0), (sp + 2, bp, W + 1, 2.0),
                 (sp, bp + 1, W + 1, 2.0)):
        assert argmax_rc(*args) == -1, args
    assert argmax_rc(sp, bp, W + 1, 2.0, Vv=VP + 1) == -1  # (w_ld < V: the originals' own check)
    torch.cuda.synchronize()
    assert bool((ids == -7).all()) and int(ws.abs().sum()) == 0
    for bad in (dict(penalty=0.0), dict(penalty=float("nan"))):
        cons = dict(seen=seen, banned=banned, penalty=2.0)
        cons.update(bad)
        with pytest.raises(TmiError):
            _topk(ops, x, d, w, VP, M, d, V, 6, cons=cons)
        with pytest.raises(TmiError):
            _sample(ops, x, d, w, VP, M, d, V, 8, 1.0, 1.0, 1, cons=cons)
    short = torch.zeros(M, W - 1, dtype=torch.int32, device=dev)
    for fn in (lambda k: _argmax(ops, x, d, w, VP, M, d, V, cons=k), lambda k: _topk(ops, x, d, w, VP, M, d, V, 6, cons=k),
               lambda k: _sample(ops, x, d, w, VP, M, d, V, 8, 1.0, 1.0, 1, cons=k)):
        with pytest.raises(ValueError):
            fn(dict(seen=short, banned=None, penalty=1.0))


def test_recorded_constraint_calls_replay_bit_for_bit(dev):
    """The four new entry points go through the launch-plan wrapper: recorded once (four launches), their outputs
    overwritten, replayed with zero deltas - the same bits as the direct calls."""
    ops, _ = _mods()
    from tethys_speech_amd import plan
    d, V, M = 64, 130, 3
    c = R.head_case(d, V, M)
    VP, W = c["VP"], R.words(V)
    x, w = torch.from_numpy(c["x"]).to(dev), torch.from_numpy(c["w"]).to(dev)
    cons = dict(seen=_bits(c["seen"], dev), banned=_bits(c["banned"], dev), penalty=2.0)
    sc = R.set_case(M, V, 40, 2)
    prefix, static = torch.from_numpy(sc["prefix"]).to(dev), _bits(R.set_case_static(R.set_case(1, V, 40, 2)), dev)
    i32 = dict(dtype=torch.int32, device=dev)
    sets = torch.empty(2, M, W, **i32)
    a_ids, a_cnt = torch.empty(M, **i32), torch.empty(1, **i32)
    k_ids, k_lp, k_lse = torch.empty(M, 6, **i32), torch.empty(M, 6, device=dev), torch.empty(M, device=dev)
    s_ids, s_lp, s_fin, s_cnt = torch.empty(M, **i32), torch.empty(M, device=dev), torch.zeros(M, **i32), torch.empty(1, **i32)
    outs = [sets, a_ids, a_cnt, k_ids, k_lp, k_lse, s_ids, s_lp, s_cnt]
    ws = [torch.zeros(M + 1, dtype=torch.int64, device=dev),
          torch.zeros(ops.lm_head_topk_workspace_elems(M, V, 6), dtype=torch.int64, device=dev),
          torch.zeros(ops.lm_head_sample_workspace_elems(M, V, 8), dtype=torch.int64, device=dev)]

    def reset():
        for t in outs:
            t.view(torch.uint8).fill_(0x5A)
        s_fin.zero_()

    def run():
        ops.decode_constraints(prefix, sc["ld"], M, 40, V, sets[0], sets[1], ngram=2, static_banned=static)
        ops.lm_head_argmax_c(x, d, w, VP, M, d, V, a_ids, 1, ws[0], eos_id=3, eos_count=a_cnt, **cons)
        ops.lm_head_topk_c(x, d, w, VP, M, d, V, 6, k_ids, k_lp, ws[1], lse=k_lse, **cons)
        ops.lm_head_sample_c(x, d, w, VP, M, d, V, s_ids, 1, s_fin, s_cnt, ws[2], top_k=8, top_p=0.9, seed=4, eos_id=3,
                             pad_id=3, logprob=s_lp, **cons)

    def snap():
        torch.cuda.synchronize()
        return [t.clone() for t in outs + [s_fin]]

    def same(a, b):
        return all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(a, b))

    reset()
    sentinel = snap()
    run()
    eager = snap()
    assert not same(eager[:len(outs)], sentinel[:len(outs)])
    p = plan.LaunchPlan()
    reset()
    with p.recording():
        before = p.launches
        run()
        assert p.launches == before + 4
    assert same(snap(), eager)
    reset()
    p.replay(0, 0)
    assert same(snap(), eager) and all(int(t.abs().sum()) == 0 for t in ws)
