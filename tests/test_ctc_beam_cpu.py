"""The reference and the bound of tests/_ctc_beam_ref.py, and the host side of the beam decoder, without a GPU: the float64
prefix beam search against the CTC forward recursion and torch's ctc_loss over EVERY sequence that has a path (nothing is
pruned at K = 16 there, so a beam's score is the sequence's whole log-likelihood), the listed mutations each caught, the
bound against an honest fp32 transcription, the decidedness of every exact-tier case that the GPU tests use,
check_ctc_beam_args' refusals and the new symbols of the binding."""
import itertools

import numpy as np
import pytest

import _ctc_beam_ref as R
import _ctc_ref as C

_CACHE = {}


def case(c):
    """(lp, the float64 reference) of an exact-tier case, computed once."""
    if c[0] not in _CACHE:
        lp = R.case_lp(c)
        _CACHE[c[0]] = (lp, R.beam_ref(lp, c[3]))
    return _CACHE[c[0]]


def by_name(name):
    return next(c for c in R.EXACT_CASES if c[0] == name)


def sequences_with_a_path(V, T, blank=0):
    syms = [v for v in range(V) if v != blank]
    out = []
    for L in range(T + 1):
        for seq in itertools.product(syms, repeat=L):
            if C.min_frames(np.array(seq, dtype=np.int64)) <= T:
                out.append(seq)
    return out


def differs(got, ref):
    """Would the checks of the exact tier fail?  Tokens, lengths, n_beams equal; every score within its bound."""
    if got["tokens"] != ref["tokens"] or got["n_beams"] != ref["n_beams"]:
        return True
    return bool((np.abs(got["scores"] - ref["scores"]) > ref["bounds"]).any())


# ------------------------------------------------------------------------------------------------ the exhaustive pin
@pytest.mark.parametrize("V,T,seed", [(3, 3, 1), (2, 8, 4)])
def test_reference_returns_every_sequence_with_its_whole_likelihood(V, T, seed):
    lp = C.lp_inputs(T, V, seed)
    ref = R.beam_ref(lp, 16)
    want = sequences_with_a_path(V, T)
    assert len(want) == (9 if V == 3 else 5) and sorted(ref["tokens"]) == sorted(want) and ref["n_beams"] == len(want)
    assert (np.diff(ref["scores"]) <= 0).all()
    for seq, score, bound in zip(ref["tokens"], ref["scores"], ref["bounds"]):
        fwd = C.ctc_forward_ref(lp, np.array(seq, dtype=np.int64), T)
        assert abs(score + fwd["nll"]) <= bound + fwd["bound"], (seq, score, fwd)
        assert abs(score + fwd["nll"]) <= 1e-12 * max(abs(score), 1.0)      # two float64 sums of the same paths
        assert abs(score + C.torch_ctc(lp, np.array(seq, dtype=np.int64), T)) <= 1e-9 * max(abs(score), 1.0), seq
    total = np.logaddexp.reduce(ref["scores"])    # every path belongs to one sequence
    assert abs(total - np.logaddexp.reduce(lp, axis=1).sum()) <= 1e-9


def test_reference_without_frames_is_the_start_state():
    ref = R.beam_ref(np.zeros((0, 4)), 3, 0)
    assert ref["tokens"] == [()] and ref["scores"].tolist() == [0.0] and ref["n_beams"] == 1 and ref["decided"]


# ------------------------------------------------------------------------------------------------------- mutations
def tie_lp():
    """Every log-prob -1 (exact in fp32): the stay candidate and the two extensions of frame 0 tie."""
    return np.full((1, 3), -1.0)


def test_the_tie_rule_prefers_the_lower_candidate_index():
    ref = R.beam_ref(tie_lp(), 2)
    assert ref["tokens"] == [(), (1,)] and ref["scores"].tolist() == [-1.0, -1.0] and not ref["decided"]


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutation_breaks_a_check(mutation):
    if mutation == "tie_reversed":
        assert R.beam_ref(tie_lp(), 2, mutate=mutation)["tokens"] == [(2,), (1,)]
        return
    name = {"no_merge": "V3 K16 T3", "parent_id": "V3 K3 T48 recreated", "ce_tot": "V3 K16 T3", "keep_inf": "neginf V4 K8 T6"}[mutation]
    c = by_name(name)
    lp, ref = case(c)
    if mutation == "keep_inf":   # the first two frames: later every rank is filled with finite scores either way
        lp = lp[:2]
        ref = R.beam_ref(lp, c[3])
        assert ref["decided"] and ref["n_beams"] < c[3]
    for dtype in (np.float64, np.float32):
        assert differs(R.beam_ref(lp, c[3], dtype=dtype, mutate=mutation), ref), (mutation, dtype)
    if mutation == "parent_id":   # the silent failure of a trie-id identity: the same sequence on two ranks
        for n in R.RECREATED_CASES:
            lp, ref = case(by_name(n))
            bad = R.beam_ref(lp, by_name(n)[3], mutate=mutation)
            assert differs(bad, ref), n
        assert any(len(set(R.beam_ref(case(by_name(n))[0], by_name(n)[3], mutate=mutation)["tokens"])) < by_name(n)[3]
                   for n in R.RECREATED_CASES)
    if mutation == "no_merge":
        assert len(set(R.beam_ref(lp, c[3], mutate=mutation)["tokens"])) < 9
    if mutation == "keep_inf":
        assert R.beam_ref(lp, 8, T=1, mutate=mutation)["n_beams"] == 4 and R.beam_ref(lp, 8, T=1)["n_beams"] == 3


# --------------------------------------------------------------------------------------- the exact tier is decided
@pytest.mark.parametrize("c", R.EXACT_CASES, ids=lambda c: c[0])
def test_exact_case_is_decided_and_admits_the_fp32_transcription(c):
    lp, ref = case(c)
    name, kind, V, K, T, seed, boost = c
    assert lp.shape == (T, V) and ref["decided"] and ref["min_margin"] > 1.0, (name, ref["min_margin"])
    assert len(set(ref["tokens"])) == ref["n_beams"] <= K and (np.diff(ref["scores"]) < 0).all()
    f32 = R.beam_ref(lp, K, dtype=np.float32)
    assert f32["tokens"] == ref["tokens"] and f32["n_beams"] == ref["n_beams"]
    r = C.ratio(f32["scores"], ref["scores"], ref["bounds"])
    print(f"ctc beam {name}: fp32 numpy at {r:.4f} of the bound, smallest gap {ref['min_margin']:.2f} of its bounds, "
          f"{ref['n_merges']} folds, {ref['n_recreated_merges']} into recreated prefixes")
    assert r <= 1.0
    assert (ref["bounds"] <= 1e-4 * np.maximum(np.abs(ref["scores"]), 1.0)).all()    # the bound is not vacuous
    for seq, s in zip(f32["tokens"], f32["scores"]):   # pruning only loses mass
        assert s <= -C.ctc_forward_ref(lp, np.array(seq, dtype=np.int64), T)["nll"] + R.pruned_score_bound(lp, T)


def test_exact_tier_covers_the_classes():
    cs = R.EXACT_CASES
    assert {c[3] for c in cs} == {1, 2, 3, 4, 8, 16} and {c[2] for c in cs} >= {3, 32, 64}
    assert min(c[4] for c in cs) == 1 and max(c[4] for c in cs) >= 64
    assert any(c[3] == 8 and c[4] >= 32 for c in cs) and any(c[3] == 16 and c[4] >= 32 for c in cs)
    recreated = [c[0] for c in cs if c[2] == 3 and case(c)[1]["n_recreated_merges"] > 0]
    assert len(recreated) >= 2 and set(R.RECREATED_CASES) <= set(recreated)
    assert all(case(by_name(n))[1]["n_idmiss_merges"] > 0 for n in R.RECREATED_CASES)
    few = by_name("T1 V3 K4")
    assert few[4] == 1 and few[3] > few[2] and case(few)[1]["n_beams"] == 3
    lp, ref = case(by_name("neginf V4 K8 T6"))
    assert np.isneginf(lp).any() and np.isneginf(lp[1, 1:]).all() and ref["n_beams"] >= 1
    assert R.beam_ref(lp, 8, T=2)["n_beams"] < 8      # after the frame whose non-blanks are all -inf


def test_near_uniform_inputs_are_not_decidable():
    """Why the exact tier is peaky: plain log-softmax rows at K = 16 leave gaps below the bounds."""
    assert not R.beam_ref(C.lp_inputs(300, 64, 5), 16, T=120)["decided"]


# ------------------------------------------------------------------------------------------------- the host side
def _W():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2 as W
    return W


def test_check_ctc_beam_args():
    W = _W()
    cfg = W.make_config("tiny")
    assert W.check_ctc_beam_args(cfg, None) == (1, 1) and W.check_ctc_beam_args(cfg, 1, 1) == (1, 1)
    assert W.check_ctc_beam_args(cfg, 16, 16) == (16, 16) and W.check_ctc_beam_args(cfg, np.int64(4), 2) == (4, 2)
    for kw in (dict(num_beams=0), dict(num_beams=17), dict(num_beams=-1), dict(num_beams=4.0), dict(num_beams=True),
               dict(num_beams=4, num_return_sequences=5), dict(num_beams=4, num_return_sequences=0),
               dict(num_beams=None, num_return_sequences=2), dict(num_beams=4, num_return_sequences=1.0)):
        with pytest.raises(ValueError):
            W.check_ctc_beam_args(cfg, **kw)
    with pytest.raises(ValueError):
        W.check_ctc_beam_args(W.make_config("tiny", vocab_size=65), 4)
    assert W.CTC_MAX_BEAMS == 16 and W.CTC_MAX_FRAMES == 4096 and W.CTC_MAX_LABELS == 511


def test_binding_has_the_beam_symbols_and_the_same_abi():
    import os
    import re
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops
    assert _lib.ABI_VERSION == 31
    assert len(_lib.SIGNATURES["tmi_ctc_beam"][1]) == 16 and len(_lib.SIGNATURES["tmi_ctc_beam_workspace_bytes"][1]) == 3
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tethys_mi.h")).read()
    for name, (_, args) in (("tmi_ctc_beam", _lib.SIGNATURES["tmi_ctc_beam"]),
                            ("tmi_ctc_beam_workspace_bytes", _lib.SIGNATURES["tmi_ctc_beam_workspace_bytes"])):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in include/tethys_mi.h"
        assert len(m.group(1).split(",")) == len(args), name
    lib = _lib.lib()
    assert lib.tmi_ctc_beam_workspace_bytes(2, 4, 100) == 2 * 4 * 100 * 8
    for bad in ((0, 4, 100), (65536, 4, 100), (2, 0, 100), (2, 17, 100), (2, 4, 0), (2, 4, 65537)):
        assert lib.tmi_ctc_beam_workspace_bytes(*bad) == -1, bad
    assert ops.ctc_beam_workspace_elems(2, 4, 100) == 1600
    with pytest.raises(ValueError):
        ops.ctc_beam_workspace_elems(2, 17, 100)
    assert callable(ops.ctc_beam)
