"""The references and bounds of tests/_ctc_ref.py, and the host side of Wav2Vec2ForCTC, without a GPU: the float64 forward
recursion against torch's ctc_loss, the Viterbi reference against a brute force over all paths and on gridded inputs, the
bound of the recursion against an honest fp32 transcription and against the listed mutations, check_ctc_args' refusals,
the CTC arena's names and the new symbols of the binding."""
import math

import numpy as np
import pytest
import torch

import _ctc_ref as C

CASES = C.forward_cases()
_CACHE = {}


def case(c):
    """(lp, labels, T, the float64 reference) of a shape class, computed once."""
    if c[0] not in _CACHE:
        lp, lab, T = C.case_inputs(c)
        _CACHE[c[0]] = (lp, lab, T, C.ctc_forward_ref(lp, lab, T))
    return _CACHE[c[0]]


@pytest.mark.parametrize("c", CASES, ids=lambda c: c[0])
def test_forward_reference_equals_torch_ctc_loss(c):
    lp, lab, T, ref = case(c)
    want = C.torch_ctc(lp, lab, T)
    if math.isinf(want):
        assert ref["nll"] == math.inf and ref["infeasible"] == 1
        assert "infeasible" in c[0] or "short" in c[0]
    else:
        assert ref["infeasible"] == 0 and abs(ref["nll"] - want) <= 1e-9 * abs(want), (ref["nll"], want)
        assert not ("infeasible" in c[0] or "short" in c[0])


def test_forward_reference_without_frames_is_infeasible():
    assert C.ctc_forward_ref(np.zeros((0, 4)), [1], 0)["infeasible"] == 1


@pytest.mark.parametrize("c", CASES, ids=lambda c: c[0])
def test_bound_admits_the_fp32_transcription(c):
    lp, lab, T, ref = case(c)
    f32 = C.ctc_forward_ref(lp, lab, T, dtype=np.float32)
    assert f32["infeasible"] == ref["infeasible"]
    if ref["infeasible"]:
        assert f32["nll"] == ref["nll"] == math.inf
    else:
        r = abs(f32["nll"] - ref["nll"]) / ref["bound"]
        print(f"ctc forward {c[0]}: fp32 numpy at {r:.4f} of the bound {ref['bound']:.3e}")
        assert r <= 1.0
        assert ref["bound"] <= 1e-4 * max(abs(ref["nll"]), 1.0)  # the bound is not vacuous


# mutation -> a shape class that is built to show it
MUTANT_CASE = {"skip_equal": "T65 L20 equal", "skip_blank": "T65 L31", "final_one": "T65 L31", "frame_more": "T65 L31",
               "frame_less": "T65 L31", "max": "T65 L31"}


@pytest.mark.parametrize("mutation", C.MUTATIONS)
def test_bound_rejects_mutation(mutation):
    c = next(x for x in CASES if x[0] == MUTANT_CASE[mutation])
    lp, lab, T, ref = case(c)
    bad = C.ctc_forward_ref(lp, lab, T, dtype=np.float32, mutate=mutation)
    assert bad["infeasible"] != ref["infeasible"] or abs(bad["nll"] - ref["nll"]) > ref["bound"], (mutation, bad, ref)


def test_mutations_change_feasibility_where_the_rule_decides_it():
    """Skipping across equal labels makes 'one short' feasible: an exact output changes."""
    c = next(x for x in CASES if x[0] == "T38 L20 equal short")
    lp, lab, T, ref = case(c)
    assert ref["infeasible"] == 1 and C.ctc_forward_ref(lp, lab, T, mutate="skip_equal")["infeasible"] == 0
    assert C.ctc_forward_ref(lp, lab, T, mutate="frame_more")["infeasible"] == 0


# ------------------------------------------------------------------------------------------------------ Viterbi
@pytest.mark.parametrize("T,labels", [(1, []), (3, []), (1, [2]), (4, [2]), (6, [2, 3]), (6, [2, 2]), (5, [3, 1]), (3, [2, 2]),
                                      (2, [2, 2])])
def test_viterbi_reference_equals_brute_force(T, labels):
    lp = C.lp_inputs(T, 5, seed=T * 11 + len(labels))
    ref = C.viterbi_ref(lp, labels, T)
    best = C.viterbi_brute(lp, labels)
    if best == -math.inf:
        assert ref["infeasible"] == 1 and ref["total"] == -math.inf and (ref["start"] == -1).all()
        return
    assert ref["infeasible"] == 0 and abs(ref["total"] - best) <= 1e-12 * abs(best)
    assert C.path_problems(ref["states"], labels, T, ref["start"], ref["end"]) == []
    assert abs(C.path_score(lp, labels, ref["states"]) - best) <= 1e-12 * abs(best)


def test_viterbi_tie_rule_by_hand():
    """All-zero log-probs: every comparison ties.  stay beats step beats skip, and the end state is S-1."""
    z = np.zeros((3, 4))
    r = C.viterbi_ref(z, [2], 3)
    assert r["states"].tolist() == [1, 2, 2] and r["start"].tolist() == [0] and r["end"].tolist() == [1] and r["total"] == 0.0
    # S = 5, the end state is 4.  Walking back: state 4 stays while it was reachable a frame earlier (from t = 2), then steps
    # to 3; state 3 was not reachable at t = 0 and neither was 2, so the move into (1, 3) is the skip from state 1
    r = C.viterbi_ref(np.zeros((4, 4)), [2, 3], 4)
    assert r["states"].tolist() == [1, 3, 4, 4]
    other = C.viterbi_ref(z, [2], 3, ties="last")
    assert other["states"].tolist() != C.viterbi_ref(z, [2], 3)["states"].tolist()


@pytest.mark.parametrize("T,L,kind", [(40, 7, "random"), (70, 33, "alt"), (65, 20, "equal")])
def test_viterbi_gridded_inputs_are_exact_in_fp32(T, L, kind):
    """On the grid k / 64 every fp32 sum is exact: the fp32 transcription equals the float64 reference, ties included; on a
    coarse grid most comparisons tie, and resolving ties the other way changes the path."""
    lab = C.labels_for(kind, L, 32, seed=T)
    for lp in (C.grid_lp(T, 32, seed=L), np.round(C.grid_lp(T, 32, seed=L + 1) / 8)):
        a, b = C.viterbi_ref(lp, lab, T), C.viterbi_ref(lp, lab, T, dtype=np.float32)
        assert a["total"] == b["total"] and np.array_equal(a["states"], b["states"])
        assert np.array_equal(a["start"], b["start"]) and np.array_equal(a["end"], b["end"])
        assert C.path_problems(a["states"], lab, T, a["start"], a["end"]) == []
        assert C.path_score(lp, lab, a["states"]) == a["total"]
    coarse = np.round(C.grid_lp(T, 32, seed=L + 1) / 8)
    assert not np.array_equal(C.viterbi_ref(coarse, lab, T, ties="last")["states"], C.viterbi_ref(coarse, lab, T)["states"])


def test_viterbi_total_is_below_the_forward_likelihood():
    c = next(x for x in CASES if x[0] == "T65 L31")
    lp, lab, T, ref = case(c)
    assert C.viterbi_ref(lp, lab, T)["total"] < -ref["nll"]


# ------------------------------------------------------------------------------------- log-softmax and greedy refs
def test_logsoftmax_reference_and_bound():
    x = C.logits_inputs(9, 33, seed=4)
    x[2, :] = 1.25          # equal logits: argmax 0
    x[3, 7] = 3.0e4         # one dominating value
    x[4, 5:9] = -np.inf
    logp, amax, bound = C.logsoftmax_ref(x)
    want = torch.log_softmax(torch.from_numpy(x), dim=1).numpy()
    assert np.allclose(logp[np.isfinite(want)], want[np.isfinite(want)], rtol=1e-12, atol=1e-12)
    assert (logp[4, 5:9] == -np.inf).all() and amax[2] == 0 and amax[3] == 7
    x32 = x.astype(np.float32)
    m = x32.max(axis=1, keepdims=True)
    got = x32 - (m + np.log(np.exp(x32 - m).sum(axis=1, keepdims=True, dtype=np.float32)))
    assert C.ratio(got, logp, bound) <= 1.0
    off = np.where(np.isfinite(got), got * np.float32(1 + 3e-6), got)
    assert C.ratio(off, logp, bound) > 1.0   # 50 ulps off is outside


def test_greedy_reference_and_bound():
    a = np.array([0, 3, 3, 0, 3, 4, 4, 4, 0, 0, 5])
    lp = C.lp_inputs(len(a), 8, seed=2)
    g = C.greedy_ref(a, lp, len(a), 0)
    assert g["tokens"].tolist() == [3, 3, 4, 5] and g["start"].tolist() == [1, 4, 5, 10] and g["end"].tolist() == [3, 5, 8, 11]
    g = C.greedy_ref(a, lp, 7, 0)   # a shorter clip: the run of 4 ends with it
    assert g["tokens"].tolist() == [3, 3, 4] and g["end"].tolist() == [3, 5, 7]
    a = np.random.default_rng(0).integers(0, 8, size=700)
    lp = C.lp_inputs(700, 8, seed=3)
    g = C.greedy_ref(a, lp, 700, 0)
    assert abs(C.greedy_best_f32(a, lp, 700) - g["best"]) <= g["best_bound"] < 1e-5 * abs(g["best"])


def test_levenshtein_forms_agree():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2 as W
    g = np.random.default_rng(5)
    for _ in range(40):
        h, r = g.integers(1, 5, size=g.integers(0, 12)), g.integers(1, 5, size=g.integers(0, 12))
        assert W.edit_distance(h, r) == C.levenshtein(h.tolist(), r.tolist())
    assert W.edit_distance([1, 2, 3], [1, 2, 3]) == 0 and W.edit_distance([], [1, 2]) == 2


# ------------------------------------------------------------------------------------------------- the host side
def _W():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2 as W
    return W


def test_check_ctc_args_refusals():
    W = _W()
    cfg = W.make_config("tiny")
    T = W.frame_lengths(cfg, [4000])[0]
    ok = torch.ones(2, T)
    ok[1, T - 3:] = 0
    B, Tn, fl, mask, lab, lens = W.check_ctc_args(cfg, (2, 4000), [[1, 2, 3], [4, 5, 0]], [3, 2], ok)
    assert (B, Tn) == (2, T) and fl.tolist() == [T, T - 3] and lab.dtype == np.int32 and lens.tolist() == [3, 2]
    assert W.check_ctc_args(cfg, (2, 4000))[2].tolist() == [T, T]
    assert W.check_ctc_args(cfg, (1, 4000), torch.zeros(1, 0, dtype=torch.int64))[4].shape == (1, 1)   # L_max = 0
    bad_mask = ok.clone()
    bad_mask[0, 2] = 0          # a hole: not a prefix
    half = ok.clone()
    half[0, 1] = 0.5
    empty = ok.clone()
    empty[1] = 0
    for kw in (dict(labels=[[1, 2, 32], [1, 2, 3]]),                      # outside [0, V)
               dict(labels=[[1, -1, 3], [1, 2, 3]]),
               dict(labels=[[1, 0, 3], [1, 2, 3]]),                       # the blank inside the length
               dict(labels=[[1, 2, 3], [1, 2, 3]], label_lengths=[3, 4]),  # a length past L_max
               dict(labels=[[1, 2, 3], [1, 2, 3]], label_lengths=[3]),
               dict(labels=torch.ones(2, 512, dtype=torch.int64)),          # L > 511
               dict(labels=torch.ones(3, 4, dtype=torch.int64)),            # another batch
               dict(labels=torch.ones(2, 4)),                               # not integer
               dict(label_lengths=[1, 1]),                                  # lengths without labels
               dict(attention_mask=bad_mask), dict(attention_mask=half), dict(attention_mask=empty),
               dict(attention_mask=torch.ones(2, T + 1))):
        with pytest.raises(ValueError):
            W.check_ctc_args(cfg, (2, 4000), **kw)
    with pytest.raises(ValueError):
        W.check_ctc_args(W.make_config("tiny", vocab_size=65), (2, 4000))
    with pytest.raises(ValueError):
        W.check_ctc_args(W.make_config("tiny", ctc_blank_id=32), (2, 4000))
    assert W.check_ctc_args(cfg, (2, 4000), [[1, 0], [1, 2]], [1, 2])[5].tolist() == [1, 2]  # the blank past the length is fine


def test_config_defaults_and_frame_seconds():
    W = _W()
    cfg = W.Wav2Vec2Config()
    assert (cfg.vocab_size, cfg.ctc_blank_id, cfg.ctc_loss_reduction, cfg.ctc_zero_infinity) == (32, 0, "sum", False)
    assert W.frame_seconds(cfg) == 320 / 16000


def test_ctc_arena_shares_the_base_names():
    W = _W()
    cfg = W.make_config("tiny", vocab_size=29)
    pre, ctc = W.W2VArena(cfg, "cpu"), W.W2VArena(cfg, "cpu", head="ctc")
    assert W.W2VArena(cfg, "cpu").names == pre.names  # the default is the pre-training arena
    heads = ("quantizer.", "project_q.", "project_hid.")
    base = [n for n in pre.names if not n.startswith(heads)]
    assert ctc.names == base + ["lm_head.kernel", "lm_head.bias"]
    assert all(ctc.shapes[n] == pre.shapes[n] for n in base)
    assert ctc.shapes["lm_head.kernel"] == (cfg.hidden_size, 29) and ctc.shapes["lm_head.bias"] == (29,)
    assert not any(n.startswith(heads) for n in ctc.names)
    shared = set(pre.ref_views(pre.p)) & set(ctc.ref_views(ctc.p))
    assert shared == {k for k in pre.ref_views(pre.p) if not k.startswith(heads)}
    with pytest.raises(ValueError):
        W.W2VArena(cfg, "cpu", head="xvector")


def test_binding_has_the_ctc_symbols_and_the_same_abi():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib
    for name in ("tmi_ctc_logsoftmax", "tmi_ctc_greedy", "tmi_ctc_forward", "tmi_ctc_viterbi", "tmi_ctc_workspace_bytes"):
        assert name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 31
    assert len(_lib.SIGNATURES["tmi_ctc_forward"][1]) == 14 and len(_lib.SIGNATURES["tmi_ctc_viterbi"][1]) == 18


def test_factory_types():
    W = _W()
    for t in ("xvector", "classification"):
        with pytest.raises(NotImplementedError):
            W.create_full_model(t, "tiny", device="cpu")
