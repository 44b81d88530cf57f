"""The reference and the bound of tests/_ctc_lm_ref.py, and the host side of the LM-fused beam decoder, without a GPU: the
float64 fused search against brute force (exact CTC log-likelihood + alpha LM + beta length over EVERY sequence that has a
path, nothing pruned at K = 16), zero weights against the unfused reference, the decidedness of every exact-tier case the
GPU tests use, the bound against an honest fp32 transcription, every listed mutation caught, ``ngram_lm_table`` against
hand counts, ``check_ctc_lm_args``' refusals and the new symbol of the binding."""
import itertools
import math
import os
import re

import numpy as np
import pytest

import _ctc_beam_ref as R
import _ctc_lm_ref as L
import _ctc_ref as C


def by_name(name):
    return next(c for c in L.LM_CASES if c[0] == name)


def lg(p):
    """log p as the table holds it: float64 logs rounded to fp32."""
    return pytest.approx(math.log(p), rel=2.0 ** -22, abs=2.0 ** -30)


def sequences_with_a_path(V, T, blank=0):
    syms = [v for v in range(V) if v != blank]
    return [seq for n in range(T + 1) for seq in itertools.product(syms, repeat=n)
            if C.min_frames(np.array(seq, dtype=np.int64)) <= T]


# ------------------------------------------------------------------------------------------------ the exhaustive pin
def lm_logprob(seq, lm, order, V, blank):
    lm = lm.reshape(-1, V)
    ctx, total = L.start_ctx(V, order, blank), 0.0
    for c in seq:
        total += lm[ctx, c]
        ctx = (ctx * V + c) % V ** (order - 1)
    return total


@pytest.mark.parametrize("T,n_seq", [(3, 9), (4, 15)])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_reference_ranks_every_sequence_by_likelihood_plus_lm_plus_length(T, n_seq, order):
    V, K, alpha, beta = 3, 16, 0.75, -0.5
    lp = C.lp_inputs(T, V, 1 + T)
    lm = L.lm_table(V, order, 40 + order)
    ref = L.beam_lm_ref(lp, K, lm, order, alpha, beta)
    want = {}
    for seq in sequences_with_a_path(V, T):
        ll = -C.ctc_forward_ref(lp, np.array(seq, dtype=np.int64), T)["nll"]
        want[seq] = (ll, alpha * lm_logprob(seq, lm, order, V, 0) + beta * len(seq))
    assert len(want) == n_seq and ref["n_beams"] == n_seq
    ranked = sorted(want, key=lambda s: -(want[s][0] + want[s][1]))
    assert ref["tokens"] == ranked and (np.diff(ref["scores"]) < 0).all()
    for r, seq in enumerate(ranked):
        ll, g = want[seq]
        assert abs(ref["ctc_scores"][r] - ll) <= 1e-12 * max(abs(ll), 1.0), seq
        assert abs(ref["lm_scores"][r] - g) <= 1e-12 * max(abs(g), 1.0), seq
        assert abs(ref["scores"][r] - (ll + g)) <= 1e-12 * max(abs(ll + g), 1.0), seq
    # the ranking is not the unfused one: the LM decides something here
    assert R.beam_ref(lp, K)["tokens"] != ref["tokens"]


def test_forbidden_transitions_remove_their_sequences():
    V, T, order = 3, 4, 2
    lp = C.lp_inputs(T, V, 5)
    lm = L.lm_table(V, order, 41)
    lm[1, 2] = -np.inf                      # 2 never follows 1
    ref = L.beam_lm_ref(lp, 16, lm, order, 0.5, 0.0)
    allowed = [s for s in sequences_with_a_path(V, T) if not any(a == 1 and b == 2 for a, b in zip(s, s[1:]))]
    assert sorted(ref["tokens"]) == sorted(allowed) and len(allowed) < 15 and ref["n_forbidden"] > 0
    for seq, s in zip(ref["tokens"], ref["ctc_scores"]):     # the others keep their whole likelihood
        assert abs(s + C.ctc_forward_ref(lp, np.array(seq, dtype=np.int64), T)["nll"]) <= 1e-12 * max(abs(s), 1.0)
    # alpha = 0 does not lift a ban
    assert sorted(L.beam_lm_ref(lp, 16, lm, order, 0.0, 0.0)["tokens"]) == sorted(allowed)


@pytest.mark.parametrize("name", ["V3 K16 T3", "V3 K3 T48 recreated", "V32 K4 T100", "neginf V4 K8 T6", "V32 K8 T32"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zero_weights_reproduce_the_unfused_reference(name, dtype):
    c = next(x for x in R.EXACT_CASES if x[0] == name)
    lp = R.case_lp(c)
    plain = R.beam_ref(lp, c[3], dtype=dtype)
    for order in (1, 2):
        fused = L.beam_lm_ref(lp, c[3], L.lm_table(c[2], order, 9), order, 0.0, 0.0, dtype=dtype)
        assert fused["tokens"] == plain["tokens"] and fused["n_beams"] == plain["n_beams"]
        assert (fused["scores"] == plain["scores"]).all() and (fused["ctc_scores"] == plain["scores"]).all()
        assert (fused["lm_scores"] == 0).all() and (fused["lm_bounds"] == 0).all()


def test_fma32_is_the_correctly_rounded_fma():
    from fractions import Fraction
    g = np.random.default_rng(3)
    vals = g.standard_normal((2000, 3)).astype(np.float32) * np.float32(2.0) ** g.integers(-20, 20, (2000, 3)).astype(np.float32)
    # cases built to sit on a double-rounding edge: a b exactly half an ulp of c, plus a crumb
    vals[:50, 0], vals[:50, 1] = np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -25 + 2.0 ** -48)
    vals[:50, 2] = np.float32(1.0) + np.arange(50, dtype=np.float32) * np.float32(2.0 ** -23)
    for a, b, c in vals:
        exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        got = L.fma32(a, b, c)
        lo, hi = np.nextafter(got, np.float32(-np.inf)), np.nextafter(got, np.float32(np.inf))
        d = abs(Fraction(float(got)) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact), (a, b, c)
    if hasattr(math, "fma"):
        assert all(float(L.fma32(a, b, c)) == float(np.float32(math.fma(float(a), float(b), float(c)))) for a, b, c in vals[50:])


# --------------------------------------------------------------------------------------- the exact tier is decided
@pytest.mark.parametrize("case", L.LM_CASES, ids=lambda c: c[0])
def test_exact_case_is_decided_and_admits_the_fp32_transcription(case):
    (lp, lm, K, T, V, order, blank), ref = L.case_ref(case)
    assert lp.shape == (T, V) and lm.shape == (V ** (order - 1), V)
    assert ref["decided"] and ref["min_margin"] > 1.0, (case[0], ref["min_margin"])
    assert len(set(ref["tokens"])) == ref["n_beams"] <= K and (np.diff(ref["scores"]) < 0).all()
    f32 = L.beam_lm_ref(lp, K, lm, order, L.ALPHA, L.BETA, T=T, blank=blank, dtype=np.float32)
    assert f32["tokens"] == ref["tokens"] and f32["n_beams"] == ref["n_beams"]
    rs = [C.ratio(f32[s], ref[s], ref[b]) if ref["n_beams"] else 0.0
          for s, b in (("scores", "bounds"), ("ctc_scores", "ctc_bounds"), ("lm_scores", "lm_bounds"))]
    print(f"ctc lm {case[0]}: fp32 numpy at {rs[0]:.4f} / {rs[1]:.4f} / {rs[2]:.4f} of the score / ctc / lm bounds, smallest "
          f"gap {ref['min_margin']:.2f} of its bounds, {ref['n_merges']} folds, {ref['n_forbidden']} forbidden")
    assert max(rs) <= 1.0 and not L.differs(f32, ref)
    assert (ref["bounds"] <= 1e-4 * np.maximum(np.abs(ref["scores"]), 1.0)).all()    # the bound is not vacuous
    for seq, g in zip(ref["tokens"], f32["lm_scores"]):      # g is a function of the sequence alone
        assert g == float(L.g_along(seq, lm, order, L.ALPHA, L.BETA, V, blank)), seq
    for seq, s in zip(f32["tokens"], f32["ctc_scores"]):     # pruning only loses mass
        rot = np.roll(lp, -blank, axis=1) if blank else lp
        labels = np.array([(t - blank) % V for t in seq], dtype=np.int64)
        assert s <= -C.ctc_forward_ref(rot, labels, T)["nll"] + R.pruned_score_bound(lp, T)


def test_exact_tier_covers_the_classes():
    cs = L.LM_CASES
    assert len(cs) == 63 and len({c[0] for c in cs}) == 63
    assert {(c[1][0], c[2]) for c in cs[:60]} == {(b[0], o) for b in R.EXACT_CASES for o in (1, 2, 3)}
    assert all(c[4] == 0.0 and c[5] == 0 for c in cs[:60])
    neg = [c for c in cs if c[4] > 0]
    assert len(neg) == 2
    for c in neg:
        (lp, lm, K, T, V, order, blank), ref = L.case_ref(c)
        share = np.isneginf(lm).mean()
        assert 0.05 <= share <= 0.2 and ref["n_forbidden"] > 0 and ref["n_beams"] >= 1
    o4 = [c for c in cs if c[2] == 4]
    assert len(o4) == 1 and o4[0][1][2] == 8 and o4[0][5] == 7 and L.start_ctx(8, 4, 7) == 7 * 73
    # the LM changes what the search returns in most cases: the fusion is exercised, not idle
    moved = sum(L.case_ref(c)[1]["tokens"] != R.beam_ref(R.case_lp(c[1]), c[1][3])["tokens"] for c in cs[:60] if c[1][4] >= 16)
    assert moved >= 20, moved


# ------------------------------------------------------------------------------------------------------- mutations
MUTATION_CASES = {"lm_in_fold": "V3 K16 T3 o2", "lm_on_stay": "V3 K16 T3 o2", "ctx_fixed": "V3 K16 T3 o2",
                  "start_zero": "V8 K4 T48 o4 blank7", "no_beta": "V3 K16 T3 o1", "keep_neginf": "V3 K8 T16 o3 neginf"}


@pytest.mark.parametrize("mutation", L.MUTATIONS)
def test_mutation_breaks_a_check(mutation):
    assert set(MUTATION_CASES) == set(L.MUTATIONS)
    (lp, lm, K, T, V, order, blank), ref = L.case_ref(by_name(MUTATION_CASES[mutation]))
    for dtype in (np.float64, np.float32):
        bad = L.beam_lm_ref(lp, K, lm, order, L.ALPHA, L.BETA, T=T, blank=blank, dtype=dtype, mutate=mutation)
        assert L.differs(bad, ref), (mutation, dtype)
    if mutation == "keep_neginf":     # and on the larger table
        (lp, lm, K, T, V, order, blank), ref = L.case_ref(by_name("V32 K4 T100 o2 neginf"))
        assert L.differs(L.beam_lm_ref(lp, K, lm, order, L.ALPHA, L.BETA, T=T, dtype=np.float32, mutate=mutation), ref)


# ------------------------------------------------------------------------------------------------- the host side
def _W():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2 as W
    return W


def test_ngram_lm_table_against_hand_counts():
    W = _W()
    seqs, lens = [[1, 2, 1, 0], [2, 2, 0, 0]], [3, 2]        # (zeros past the lengths: never counted)
    t1 = W.ngram_lm_table(seqs, lens, 1, 3, 0)
    assert t1.dtype == np.float32 and t1.shape == (3,) and np.isneginf(t1[0])
    assert t1[1] == lg((3 / 7)) and t1[2] == lg((4 / 7))       # counts 2 and 3, + 1 each
    t2 = W.ngram_lm_table(seqs, lens, 2, 3, 0)
    want = {(0, 1): 2 / 4, (0, 2): 2 / 4, (1, 1): 1 / 3, (1, 2): 2 / 3, (2, 1): 2 / 4, (2, 2): 2 / 4}
    assert t2.shape == (3, 3) and np.isneginf(t2[:, 0]).all()
    for (a, c), p in want.items():
        assert t2[a, c] == lg((p)), (a, c)
    # the blank elsewhere: the start context is the blank's row, rows over the non-blank columns sum to 1
    t3 = W.ngram_lm_table([[0, 1, 0, 1], [1, 1]], [4, 2], 3, 3, 2, add_k=0.5)
    assert t3.shape == (3, 3, 3) and np.isneginf(t3[..., 2]).all()
    assert t3[2, 2, 0] == lg((1.5 / 3)) and t3[2, 2, 1] == lg((1.5 / 3))   # the two starts
    assert t3[2, 0, 1] == lg((1.5 / 2)) and t3[0, 1, 0] == lg((1.5 / 2))
    assert t3[1, 0, 1] == lg((1.5 / 2)) and t3[2, 1, 1] == lg((1.5 / 2))
    assert t3[0, 0, 0] == lg((0.5))                                                # an unseen row: uniform
    for t in (t2, t3, W.ngram_lm_table(seqs, lens, 4, 3, 0)):
        V = t.shape[-1]
        cols = [c for c in range(V) if not np.isneginf(t.reshape(-1, V)[0, c])]
        assert len(cols) == V - 1
        assert np.abs(np.exp(t.reshape(-1, V)[:, cols].astype(np.float64)).sum(axis=1) - 1.0).max() <= 1e-6
    t0 = W.ngram_lm_table(seqs, lens, 2, 3, 0, add_k=0.0)         # no smoothing: unseen transitions are forbidden
    assert np.isneginf(t0[1, 1]) and t0[1, 2] == 0.0 and t0[0, 1] == lg((0.5))
    for bad in (dict(order=0), dict(order=5), dict(vocab_size=65), dict(blank=3), dict(add_k=-1.0), dict(order=4, vocab_size=64 + 1)):
        kw = dict(order=2, vocab_size=3, blank=0, add_k=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            W.ngram_lm_table(seqs, lens, **kw)
    with pytest.raises(ValueError):
        W.ngram_lm_table([[1, 0]], [2], 2, 3, 0)       # the blank inside a length
    with pytest.raises(ValueError):
        W.ngram_lm_table([[1, 3]], [2], 2, 3, 0)
    # the table passes the validator
    cfg = W.make_config("tiny", vocab_size=3)
    table, order, a, b = W.check_ctc_lm_args(cfg, t3, 0.5, 0.0, 4)
    assert order == 3 and table.shape == (27,) and table.dtype.is_floating_point


def test_check_ctc_lm_args():
    import torch
    W = _W()
    cfg = W.make_config("tiny", vocab_size=8)
    V = 8
    assert W.check_ctc_lm_args(cfg, None) is None and W.check_ctc_lm_args(cfg, None, -1.0, math.nan, None) is None
    ok = np.zeros((V, V), dtype=np.float32)
    ok[0, 3] = -np.inf
    table, order, a, b = W.check_ctc_lm_args(cfg, ok, 0.5, 0.25, 4)
    assert (order, a, b) == (2, 0.5, 0.25) and table.dtype == torch.float32 and tuple(table.shape) == (V * V,)
    assert table.is_contiguous() and table.device.type == "cpu" and bool(torch.isneginf(table[3]))
    assert W.check_ctc_lm_args(cfg, ok.reshape(-1).astype(np.float64), 0, 0, 2)[1] == 2        # flat, float64, integer weights
    assert W.check_ctc_lm_args(cfg, torch.zeros(V), 1.0, -2.0, 16)[1] == 1
    assert W.check_ctc_lm_args(cfg, torch.zeros(V, V, V, V), 1.0, 0.0, 2)[1] == 4
    bad_nan, bad_inf = ok.copy(), ok.copy()
    bad_nan[1, 1], bad_inf[1, 1] = np.nan, np.inf
    for lm, alpha, beta, K in ((ok, 0.5, 0.0, None), (ok, 0.5, 0.0, 1),              # a table with the greedy path
                               (bad_nan, 0.5, 0.0, 4), (bad_inf, 0.5, 0.0, 4),
                               (np.zeros((V, V + 1), dtype=np.float32), 0.5, 0.0, 4), (np.zeros(V * V + 1, dtype=np.float32), 0.5, 0.0, 4),
                               (np.zeros((V,) * 5, dtype=np.float32), 0.5, 0.0, 4), (np.zeros((V, V), dtype=np.int64), 0.5, 0.0, 4),
                               (np.zeros((), dtype=np.float32), 0.5, 0.0, 4),
                               (ok, -0.5, 0.0, 4), (ok, math.inf, 0.0, 4), (ok, math.nan, 0.0, 4), (ok, 0.5, math.inf, 4),
                               (ok, 0.5, math.nan, 4), (ok, 1e39, 0.0, 4), (ok, "1", 0.0, 4), (ok, 0.5, None, 4), (ok, True, 0.0, 4),
                               (ok, 0.5, 0.0, 17)):
        with pytest.raises(ValueError):
            W.check_ctc_lm_args(cfg, lm, alpha, beta, K)
    big = W.make_config("tiny", vocab_size=64)
    assert W.CTC_LM_MAX_ORDER == 4 and W.CTC_LM_MAX_ENTRIES == 2 ** 24 and 64 ** 4 == W.CTC_LM_MAX_ENTRIES
    assert W.check_ctc_lm_args(big, torch.zeros(64, 64, 64), 0.5, 0.0, 4)[1] == 3


def test_binding_has_the_lm_symbol_and_the_same_abi():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops
    assert _lib.ABI_VERSION == 31
    assert "tmi_ctc_beam_lm" in _lib.SIGNATURES, "the fused beam search is not bound"
    args = _lib.SIGNATURES["tmi_ctc_beam_lm"][1]
    assert len(args) == 22 and args.count(_lib.c_f32) == 2
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tethys_mi.h")).read()
    m = re.search(r"\btmi_ctc_beam_lm\(([^;]*)\);", header)
    assert m, "tmi_ctc_beam_lm is not declared in include/tethys_mi.h"
    assert len(m.group(1).split(",")) == len(args)
    assert len(_lib.SIGNATURES["tmi_ctc_beam"][1]) == 16          # the unfused entry point is as it was
    assert hasattr(_lib.lib(), "tmi_ctc_beam_lm") and callable(ops.ctc_beam_lm)
