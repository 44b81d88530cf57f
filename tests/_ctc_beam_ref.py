"""Float64 reference, seeded inputs and bounds for tmi_ctc_beam (csrc/ctc_beam.hip), written literally from the definition
in include/tethys_mi.h.  CPU only: nothing here imports the GPU package, so tests/test_ctc_beam_cpu.py checks the reference
(against the CTC forward recursion of tests/_ctc_ref.py and torch's ctc_loss over every sequence that has a path) and the
bound (reached by an honest fp32 transcription, every listed mutation caught) before tests/test_ctc_beam_kernels_gpu.py
and tests/test_ctc_beam_gpu.py compare the kernel with it.

Identity is the token tuple itself.  Beside it every beam carries a node id as a trie would give it (a new id whenever an
extension creates a beam) and its parent's, so that the mutation "identity by parent id" can be stated and the folds
that it misses counted (``n_idmiss_merges``).

The bound is derived, not fitted, with the constants of tests/_ctc_ref.py (U, C_EXP, C_LOG, SLACK; the device's expf / logf
are assumed to meet the OpenCL accuracy, as there).  LSE is non-expansive in the sup norm, so a value's bound is the largest
bound among its finite inputs plus what the step itself rounds:
    LSE2(a, b)   the two arguments a - m, b - m (U / e each against a sum >= 1), two exp (C_EXP relative on the sum), one
                 add (U): rs = C_EXP + 2 U / e + U, an absolute rs (1 + rs) of the log; the log itself C_LOG |log s|
                 (log s <= log 2); m + log s one add: U |LSE2|
    lp + x       one add: U |lp + x|
(1 + SLACK) covers the second-order terms and the difference between the device's magnitudes and the reference's.  A
bound is carried next to every pb, pnb and score.  A frame is DECIDED when, among its finite candidates in order, every
gap between two neighbouring kept candidates and the gap between the last kept and the first dropped exceeds the sum of
the two scores' bounds: the device then keeps the same candidates in the same order, by induction over the frames its
values stay within the bounds, and tokens, lengths and n_beams are equal exactly.
"""
import math

import numpy as np

import _ctc_ref as C
from _ctc_ref import C_EXP, C_LOG, NEG, SLACK, U

RS2 = C_EXP + 2 * U / math.e + U
K_MAX, V_MAX = 16, 64


def lse2(a, b, dtype=np.float64):
    """-> (LSE2(a, b) in ``dtype``, what the step rounds)."""
    a, b = dtype(a), dtype(b)
    m = a if a >= b else b
    if m == NEG:
        return dtype(NEG), 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        s = dtype(dtype(np.exp(dtype(a - m))) + dtype(np.exp(dtype(b - m))))
        out = dtype(m + dtype(np.log(s)))
    loc = (1 + SLACK) * (RS2 * (1 + RS2) + C_LOG * abs(math.log(max(float(s), 1.0))) + U * abs(float(out)))
    return out, loc


def _pred(a, Ea, b, Eb):
    return max(Ea if a > NEG else 0.0, Eb if b > NEG else 0.0)


def _add(lpv, x, Ex, dtype):
    with np.errstate(invalid="ignore"):
        out = dtype(dtype(lpv) + dtype(x))
    if not out > NEG:
        return dtype(NEG), 0.0
    return out, Ex + (1 + SLACK) * U * abs(float(out))


MUTATIONS = ["no_merge", "parent_id", "ce_tot", "tie_reversed", "keep_inf"]


def beam_ref(lp, K, T=None, blank=0, dtype=np.float64, mutate=None):
    """lp float64 [>= T, V] (fp32-exact) -> dict(tokens: the K' sequences as tuples by rank, lengths, scores, bounds (per
    score), n_beams, decided, min_margin (the smallest gap over the sum of its two bounds), n_merges, n_recreated_merges
    (a fold into a prefix that had left the set earlier), n_idmiss_merges (a fold that identity by parent id misses)).
    ``dtype=np.float32`` is the honest fp32 transcription; ``mutate``: None or one of MUTATIONS."""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0] if T is None else min(T, lp.shape[0])
    V = lp.shape[1]
    beams = [dict(seq=(), pb=dtype(0.0), pnb=dtype(NEG), Epb=0.0, Epnb=0.0, id=0, par=-1)]
    next_id, left = 1, set()
    decided, min_margin = True, math.inf
    n_merges = n_recreated = n_idmiss = 0
    for t in range(max(T, 0)):
        row = lp[t]
        index = {b["seq"]: p for p, b in enumerate(beams)}
        stay = []
        for k, b in enumerate(beams):
            tot, loc = lse2(b["pb"], b["pnb"], dtype)
            b["tot"], b["Etot"] = tot, _pred(b["pb"], b["Epb"], b["pnb"], b["Epnb"]) + loc
            pb2, Epb2 = _add(row[blank], tot, b["Etot"], dtype)
            pnb2, Epnb2 = _add(row[b["seq"][-1]], b["pnb"], b["Epnb"], dtype) if b["seq"] else (dtype(NEG), 0.0)
            stay.append(dict(index=k, seq=b["seq"], pb=pb2, Epb=Epb2, pnb=pnb2, Epnb=Epnb2, id=b["id"], par=b["par"]))
        cands = []
        for k, b in enumerate(beams):
            e = b["seq"][-1] if b["seq"] else -1
            for c in range(V):
                if c == blank:
                    continue
                from_pb = c == e and mutate != "ce_tot"
                v, Ev = _add(row[c], b["pb"] if from_pb else b["tot"], b["Epb"] if from_pb else b["Etot"], dtype)
                target = b["seq"] + (c,)
                true_p = index.get(target)
                if mutate == "no_merge":
                    p = None
                elif mutate == "parent_id":
                    p = next((q for q, x in enumerate(beams) if x["seq"] and x["seq"][-1] == c and x["par"] == b["id"]), None)
                else:
                    p = true_p
                if true_p is not None:
                    n_merges += 1
                    n_recreated += target in left
                    n_idmiss += beams[true_p]["par"] != b["id"]
                if p is not None:
                    s = stay[p]
                    if v > NEG:
                        new, loc = lse2(s["pnb"], v, dtype)
                        s["Epnb"] = _pred(s["pnb"], s["Epnb"], v, Ev) + loc
                        s["pnb"] = new
                else:
                    cands.append(dict(index=K + k * V + c, seq=target, pb=dtype(NEG), Epb=0.0, pnb=v, Epnb=Ev, id=None,
                                      par=b["id"], score=v, E=Ev))
        for s in stay:
            s["score"], loc = lse2(s["pb"], s["pnb"], dtype)
            s["E"] = _pred(s["pb"], s["Epb"], s["pnb"], s["Epnb"]) + loc
        cands = stay + cands
        if mutate != "keep_inf":
            cands = [x for x in cands if x["score"] > NEG]
        sign = -1 if mutate == "tie_reversed" else 1
        cands.sort(key=lambda x: (-float(x["score"]), sign * x["index"]))
        finite = [x for x in cands if x["score"] > NEG]
        for i in range(min(K, len(finite) - 1)):
            gap, both = float(finite[i]["score"]) - float(finite[i + 1]["score"]), finite[i]["E"] + finite[i + 1]["E"]
            margin = gap / both if both > 0 else (math.inf if gap > 0 else 0.0)
            min_margin = min(min_margin, margin)
            decided = decided and margin > 1.0
        kept = cands[:K]
        for x in kept:
            if x["id"] is None:
                x["id"], next_id = next_id, next_id + 1
        now = {x["seq"] for x in kept}
        left |= {b["seq"] for b in beams if b["seq"] not in now}
        beams = kept
    scores, bounds = [], []
    for b in beams:
        s, loc = lse2(b["pb"], b["pnb"], dtype)
        scores.append(float(s))
        bounds.append(_pred(b["pb"], b["Epb"], b["pnb"], b["Epnb"]) + loc)
    return {"tokens": [b["seq"] for b in beams], "lengths": [len(b["seq"]) for b in beams], "scores": np.array(scores),
            "bounds": np.array(bounds), "n_beams": len(beams), "decided": decided, "min_margin": min_margin,
            "n_merges": n_merges, "n_recreated_merges": n_recreated, "n_idmiss_merges": n_idmiss}


def same_result(a, b):
    return a["tokens"] == b["tokens"] and np.array_equal(a["scores"], b["scores"])


def pruned_score_bound(lp, T):
    """A bound on how far ABOVE -nll_float64(seq) the device's score of a sequence can lie, whatever was pruned on the way
    (the invariant tier: pruning only loses mass, so the exact value of what the device summed is <= -nll).  Every value of
    the device's recursion is the log of a sum of path probabilities, so with log-softmax rows its magnitude is at most
    M = sum_t max_c |lp[t, c]| (finite entries).  A frame takes a value through at most two LSE2 (tot or the fold, and the
    score does not feed the next frame) and one add, the end through one LSE2 more."""
    lp = np.asarray(lp, dtype=np.float64)[:T]
    M = float(np.where(np.isfinite(lp), np.abs(lp), 0.0).max(axis=1).sum()) if T > 0 else 0.0
    loc = RS2 * (1 + RS2) + C_LOG * math.log(2.0) + U * M
    return (1 + SLACK) * ((T + 1) * (2 * loc + U * M))


# ===================================================================================================== inputs
def peaky_lp(T, V, seed, boost=8.0, blank=0):
    """fp32-exact log-probabilities as float64 [T, V]: random logits plus ``boost`` on a random run-structured path (runs of
    1..4 frames, blank with probability 0.4), through logsoftmax_ref, rounded to fp32.  Near-uniform log-probs cannot be
    compared exactly: at score magnitudes of 100 and more one fp32 ulp exceeds the candidates' gaps."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((T, V)) * 1.5
    syms = [v for v in range(V) if v != blank]
    t = 0
    while t < T:
        s = blank if g.random() < 0.4 else syms[int(g.integers(0, len(syms)))]
        run = int(g.integers(1, 5))
        x[t:t + run, s] += boost
        t += run
    x = x.astype(np.float32).astype(np.float64)
    return C.logsoftmax_ref(x)[0].astype(np.float32).astype(np.float64)


def neginf_lp(T, V, seed, blank=0):
    """As ``lp_inputs`` of _ctc_ref, with -inf log-probabilities: symbol V - 1 in every frame, every non-blank in frame 1."""
    x = C.logits_inputs(T, V, seed)
    x[:, V - 1] = NEG
    if T > 1:
        x[1, [v for v in range(V) if v != blank]] = NEG
    with np.errstate(invalid="ignore"):
        return C.logsoftmax_ref(x)[0].astype(np.float32).astype(np.float64)


# (name, kind, V, K, T, seed, boost): the exact tier.  Every case is `decided` (tests/test_ctc_beam_cpu.py): the seeds of
# the K >= 8 cases and of the recreated-merge cases were chosen by a search for decided inputs, never the bound.
EXACT_CASES = [
    ("T1 V3 K4", "peaky", 3, 4, 1, 1, 8.0),            # 3 finite candidates for K = 4
    ("T1 V32 K1", "peaky", 32, 1, 1, 1, 8.0),
    ("T2 V64 K16", "peaky", 64, 16, 2, 1, 8.0),
    ("neginf V4 K8 T6", "neginf", 4, 8, 6, 1, 0.0),    # -inf log-probs: frames with fewer than K finite candidates
    ("V3 K16 T3", "plain", 3, 16, 3, 1, 0.0),          # every sequence that has a path (9)
    ("V32 K1 T40", "peaky", 32, 1, 40, 1, 8.0),
    ("V3 K2 T30", "peaky", 3, 2, 30, 1, 2.0),
    ("V32 K2 T64", "peaky", 32, 2, 64, 1, 8.0),
    ("V64 K3 T33", "peaky", 64, 3, 33, 1, 8.0),
    ("V3 K3 T48 recreated", "peaky", 3, 3, 48, 2, 2.0),
    ("V3 K4 T40 recreated", "peaky", 3, 4, 40, 2, 2.0),
    ("V32 K4 T100", "peaky", 32, 4, 100, 1, 8.0),
    ("V64 K4 T65", "peaky", 64, 4, 65, 1, 8.0),
    ("V3 K8 T16", "peaky", 3, 8, 16, 1, 4.0),
    ("V32 K8 T32", "peaky", 32, 8, 32, 1, 8.0),
    ("V64 K8 T40", "peaky", 64, 8, 40, 1, 8.0),
    ("V32 K8 T64", "peaky", 32, 8, 64, 1, 8.0),
    ("V32 K16 T32", "peaky", 32, 16, 32, 1, 8.0),
    ("V64 K16 T32", "peaky", 64, 16, 32, 1, 8.0),
    ("V32 K16 T64", "peaky", 32, 16, 64, 1, 8.0),
]
RECREATED_CASES = ("V3 K3 T48 recreated", "V3 K4 T40 recreated", "V3 K8 T16")


def case_lp(case):
    name, kind, V, K, T, seed, boost = case
    if kind == "peaky":
        return peaky_lp(T, V, seed, boost)
    if kind == "neginf":
        return neginf_lp(T, V, seed)
    if kind == "plain":
        return C.lp_inputs(T, V, seed)
    raise ValueError(kind)
