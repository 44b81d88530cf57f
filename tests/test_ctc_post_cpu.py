"""The float64 reference and the bounds of tests/_ctc_post_ref.py, checked without a GPU before any kernel is compared with
them: the reference against a brute force over all paths, its identities, its gradient against central finite differences
of ``_ctc_ref.ctc_forward_ref`` and against torch's float64 ctc_loss, the soft centres against the best path on peaky
inputs, the bounds against an honest fp32 transcription (inside) and the listed mutations (outside), and the binding of
tmi_ctc_posteriors in the built library."""
import math

import numpy as np
import pytest

import _ctc_beam_ref as BR
import _ctc_post_ref as P
import _ctc_ref as C

BLANK = 0
CASES, LONG = P.cases(), P.long_cases()
TINY_CASES = [(T, lab) for lab in ([], [1], [2], [1, 2], [1, 1], [2, 1], [1, 2, 1], [1, 1, 2], [2, 2, 2], [1, 2, 2])
              for T in range(max(C.min_frames(np.array(lab, dtype=np.int64)), 1), 7)]


@pytest.mark.parametrize("T,lab", TINY_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_reference_equals_brute_force(T, lab):
    lp = C.lp_inputs(T, 3, seed=17 * T + len(lab) + sum(lab))
    ref, brute = P.post_ref(lp, lab, T), P.post_brute(lp, lab)
    assert brute["n_paths"] >= 1 and not ref["infeasible"]
    assert abs(ref["nll"] - brute["nll"]) <= 1e-12 * max(1.0, abs(brute["nll"]))
    for k in P.KEYS:
        assert np.allclose(ref[k], brute[k], rtol=1e-11, atol=1e-13), (k, T, lab)


def test_reference_without_a_path():
    lp = C.lp_inputs(3, 3, seed=5)
    for T, lab in ((2, [1, 1]), (1, [1, 2]), (0, [1])):
        ref = P.post_ref(lp, lab, T)
        assert ref["infeasible"] == 1 and ref["nll"] == math.inf and not ref["gamma"].any() and not ref["occ"].any()
        assert not ref["grad"].any() and not ref["tok_frames"].any() and (ref["tok_center"] == -1).all()
    assert P.post_brute(lp[:2], [1, 1]) is None


@pytest.mark.parametrize("c", CASES + LONG, ids=lambda c: c[0])
def test_identities_and_the_forward_reference(c):
    lp, lab, T, ref = P.case_ref(c)
    fwd = C.ctc_forward_ref(lp, lab, T)
    assert ref["infeasible"] == fwd["infeasible"] and ref["nll"] == fwd["nll"] and ref["bound_nll"] == fwd["bound"]
    print(P.bound_report(c[0], ref))
    if ref["infeasible"]:
        return
    assert np.abs(ref["occ"].sum(axis=1) - 1.0).max() <= 1e-10               # every frame is in exactly one state
    assert (ref["tok_frames"] >= 1.0 - 1e-10).all()                           # every path gives every token a frame
    assert abs(ref["tok_frames"].sum() + ref["occ"][:, BLANK].sum() - T) <= 1e-9 * T
    assert (ref["tok_center"] >= 0).all() and (ref["tok_center"] <= T - 1).all()
    if c[5] == "exact":                                                       # a single path: gamma is 0 or 1
        assert np.abs(ref["gamma"] - np.round(ref["gamma"])).max() <= 1e-12 and np.allclose(ref["tok_frames"], 1.0)


FD_H = 1.0e-3


@pytest.mark.parametrize("T,V,lab", [(5, 4, [1, 2]), (6, 5, [3, 3, 1]), (4, 3, []), (7, 4, [1, 2, 2, 3])], ids=str)
def test_grad_equals_finite_differences_and_torch(T, V, lab):
    """nll as a function of ONE logit x[t, c] is log(sum_j e^{x_j}) - log(A e^{x} + B) with A, B >= 0 (a path reads frame t
    once).  Each term has the derivatives sigma, sigma (1 - sigma), sigma (1 - sigma)(1 - 2 sigma) with sigma in [0, 1], so
    |f'''| <= 2 / (6 sqrt 3) < 0.2 and the central difference with step h is off by at most h^2 / 6 * 0.2 = h^2 / 30
    (3.4e-8 at h = 1e-3); the float64 roundings of the two nll values add about 1e-16 * |nll| / h < 1e-11."""
    x = C.logits_inputs(T, V, seed=T * 7 + V)
    lp = C.logsoftmax_ref(x)[0]
    ref = P.post_ref(lp, lab, T)
    assert np.abs(ref["grad"].sum(axis=1)).max() <= 1e-12                     # softmax rows and occ rows both sum to 1
    fd = np.zeros((T, V))
    for t in range(T):
        for c in range(V):
            hi, lo = x.copy(), x.copy()
            hi[t, c] += FD_H
            lo[t, c] -= FD_H
            fd[t, c] = (C.ctc_forward_ref(C.logsoftmax_ref(hi)[0], lab, T)["nll"]
                        - C.ctc_forward_ref(C.logsoftmax_ref(lo)[0], lab, T)["nll"]) / (2 * FD_H)
    err = np.abs(fd - ref["grad"]).max()
    print(f"finite differences h {FD_H}: {err:.2e} of {FD_H ** 2 / 30 + 1e-10:.2e}")
    assert err <= FD_H ** 2 / 30 + 1e-10
    tg = P.torch_grad(x, lab, T)
    assert np.abs(tg - ref["grad"]).max() <= 1e-12, np.abs(tg - ref["grad"]).max()
    assert abs(C.torch_ctc(lp, lab, T) - ref["nll"]) <= 1e-12 * max(1.0, ref["nll"])


@pytest.mark.parametrize("T,boost", [(40, 8.0), (40, 16.0), (120, 16.0), (120, 24.0)], ids=str)
def test_soft_centre_is_the_best_paths_on_peaky_inputs(T, boost):
    """With eps = 1 - exp(path_logprob - ll) the best path holds 1 - eps of the probability: gamma is within eps of the
    indicator of that path, and the soft centre is a convex combination of the midpoint of the token's run on it (weight
    >= 1 - eps) and of a frame in [0, T - 1]."""
    V = 32
    lp = BR.peaky_lp(T, V, seed=T + int(boost), boost=boost)
    lab = C.greedy_ref(np.argmax(lp, axis=1), lp, T, BLANK)["tokens"]
    assert len(lab) >= 3
    ref, vit = P.post_ref(lp, lab, T), C.viterbi_ref(lp, lab, T)
    eps = 1.0 - math.exp(vit["total"] - ref["ll"])
    mid = (vit["start"] + vit["end"] - 1) / 2.0
    off = np.abs(ref["tok_center"] - mid).max()
    print(f"peaky T{T} boost {boost}: {len(lab)} tokens, eps {eps:.3e}, centres off by {off:.3e} of {eps * T:.3e} frames")
    assert 0.0 <= eps < 1.0 and off <= eps * T
    on_path = np.zeros_like(ref["gamma"])
    on_path[np.arange(T), vit["states"]] = 1.0
    assert np.abs(ref["gamma"] - on_path).max() <= eps + 1e-12


@pytest.mark.parametrize("c", CASES + LONG, ids=lambda c: c[0])
def test_fp32_transcription_is_within_the_bound(c):
    lp, lab, T, ref = P.case_ref(c)
    f32 = P.post_ref(lp, lab, T, dtype=np.float32)
    assert f32["infeasible"] == ref["infeasible"]
    fwd32 = C.ctc_forward_ref(lp, lab, T, dtype=np.float32)
    assert f32["nll"] == fwd32["nll"], "the alpha pass is not ctc_forward_ref's"
    r = P.ratios(f32, ref)
    print(f"{c[0]}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) + " of the bound;  " + P.bound_report(c[0], ref))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("m", P.MUTATIONS)
def test_every_mutation_exceeds_the_bound(m):
    for c in CASES:
        lp, lab, T, ref = P.case_ref(c)
        if ref["infeasible"]:
            continue
        r = P.ratios(P.post_ref(lp, lab, T, mutate=m), ref)
        if max(r.values()) > 1.0:
            k = max(r, key=r.get)
            print(f"{m}: caught on {c[0]} ({k} at {r[k]:.3g} of its bound)")
            return
    raise AssertionError(f"no case catches the mutation {m}")


def test_the_binding_has_the_symbol():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib
    assert _lib.ABI_VERSION == 31
    res, args = _lib.SIGNATURES["tmi_ctc_posteriors"]
    assert len(args) == 24
    h = _lib.lib()
    assert h.tmi_abi_version() == 31
    fn = h.tmi_ctc_posteriors            # the built library's symbol
    # refusals need no GPU: NULL pointers, nothing launched
    assert fn(None, 0, 0, 32, None, None, None, 0, None, None, None, None, 0, 0, None, 0, 0, None, None, 1, 1, 1, 0, None) == -1
    msg = h.tmi_last_error()
    assert b"tmi_ctc_posteriors" in msg and b"L_max <= 511" in msg and b"T_max <= 4096" in msg and b"V <= 64" in msg
