"""Float64 reference, seeded inputs and bounds for tmi_ctc_beam_lm (csrc/ctc_beam.hip): the prefix beam search of
tests/_ctc_beam_ref.py with an n-gram table and a length bonus in the ranking, written literally from the definition in
include/tethys_mi.h.  CPU only.  tests/test_ctc_lm_cpu.py checks the reference (against exact CTC log-likelihoods plus the
LM terms over every sequence that has a path) and the bound (an honest fp32 transcription stays inside, every listed
mutation is caught) before the GPU tests compare the kernel with it.

The bound extends that of _ctc_beam_ref (same constants, derived, not fitted).  The table, alpha and beta are fp32 values,
exact in float64.  Next to g a bound Eg is carried:
    f  = fmaf(alpha, l, beta)   one rounding: U |f|
    g' = g + f                  one add:      U |g'|          Eg' = Eg + (1 + SLACK) U (|f| + |g'|)
    rank = score + g            one add:      E = Escore + Eg + (1 + SLACK) U |rank|
and the outputs carry Escore (ctc_scores), Eg (lm_scores) and E (scores).  A frame is DECIDED as in _ctc_beam_ref, on the
ranks: every gap between neighbouring kept candidates, and between the last kept and the first dropped, exceeds the sum
of the two ranks' bounds.  -inf table entries are decisions on exact input values: they never cost a margin.  "A forbidden
extension is not folded" cannot be observed, so no mutation states it: the sequence it would fold into contains the
forbidden transition and therefore never became a beam.
"""
import math
import struct

import numpy as np

import _ctc_beam_ref as R
import _ctc_ref as C
from _ctc_ref import NEG, SLACK, U

MUTATIONS = ["lm_in_fold", "lm_on_stay", "ctx_fixed", "start_zero", "no_beta", "keep_neginf"]


def fma32(a, b, c):
    """fmaf(a, b, c) of three fp32 values, correctly rounded: the product is exact in float64, the sum is rounded to odd in
    float64 (two-sum gives the sign of what was lost), and 53 bits rounded to odd round to 24 bits as the exact value."""
    p = float(a) * float(b)
    c = float(c)
    s = p + c
    if not math.isfinite(s):
        return np.float32(s)
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    if err != 0.0 and not struct.unpack("<q", struct.pack("<d", s))[0] & 1:
        s = math.nextafter(s, math.inf if err > 0 else -math.inf)
    return np.float32(s)


def lm_term(alpha, l, beta, dtype, mutate=None):
    if mutate == "no_beta":
        beta = 0.0
    if dtype == np.float32:
        return fma32(alpha, l, beta)
    return dtype(float(alpha) * float(l) + float(beta))


def start_ctx(V, order, blank):
    return blank * sum(V ** i for i in range(order - 1))


def beam_lm_ref(lp, K, lm, order, alpha, beta, T=None, blank=0, dtype=np.float64, mutate=None):
    """lp float64 [>= T, V] and lm float64 [V^(order-1), V] (or any shape of V^order entries), both fp32-exact; alpha, beta
    fp32-exact.  -> dict(tokens, lengths, scores / ctc_scores / lm_scores with bounds / ctc_bounds / lm_bounds, n_beams,
    decided, min_margin, n_merges, n_forbidden).  ``dtype=np.float32``: the honest fp32 transcription."""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0] if T is None else min(T, lp.shape[0])
    V = lp.shape[1]
    lm = np.asarray(lm, dtype=np.float64).reshape(-1, V)
    mod = V ** (order - 1)
    assert lm.shape[0] == mod and 1 <= order <= 4
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    ctx0 = 0 if mutate == "start_zero" else start_ctx(V, order, blank)
    beams = [dict(seq=(), pb=dtype(0.0), pnb=dtype(NEG), Epb=0.0, Epnb=0.0, g=dtype(0.0), Eg=0.0, ctx=ctx0)]
    decided, min_margin = True, math.inf
    n_merges = n_forbidden = 0
    for t in range(max(T, 0)):
        row = lp[t]
        index = {b["seq"]: p for p, b in enumerate(beams)}
        stay = []
        for k, b in enumerate(beams):
            tot, loc = R.lse2(b["pb"], b["pnb"], dtype)
            b["tot"], b["Etot"] = tot, R._pred(b["pb"], b["Epb"], b["pnb"], b["Epnb"]) + loc
            pb2, Epb2 = R._add(row[blank], tot, b["Etot"], dtype)
            pnb2, Epnb2 = R._add(row[b["seq"][-1]], b["pnb"], b["Epnb"], dtype) if b["seq"] else (dtype(NEG), 0.0)
            g, Eg = b["g"], b["Eg"]
            if mutate == "lm_on_stay" and b["seq"]:
                l = lm[b["ctx"], b["seq"][-1]]      # (the repeated token as if it were an extension)
                g = dtype(g + lm_term(alpha, l if l > NEG else 0.0, beta, dtype))
            stay.append(dict(index=k, seq=b["seq"], pb=pb2, Epb=Epb2, pnb=pnb2, Epnb=Epnb2, g=g, Eg=Eg, ctx=b["ctx"]))
        cands = []
        for k, b in enumerate(beams):
            e = b["seq"][-1] if b["seq"] else -1
            for c in range(V):
                if c == blank:
                    continue
                l = lm[b["ctx"], c]
                forbidden = l == NEG
                n_forbidden += forbidden
                if forbidden and mutate == "keep_neginf":
                    l, forbidden = 0.0, False
                elif forbidden:
                    continue
                from_pb = c == e
                v, Ev = R._add(row[c], b["pb"] if from_pb else b["tot"], b["Epb"] if from_pb else b["Etot"], dtype)
                target = b["seq"] + (c,)
                p = index.get(target)
                if p is not None:
                    n_merges += 1
                    s = stay[p]
                    if mutate == "lm_in_fold" and v > NEG:
                        v = dtype(v + lm_term(alpha, l, beta, dtype))
                    if v > NEG:
                        new, loc = R.lse2(s["pnb"], v, dtype)
                        s["Epnb"] = R._pred(s["pnb"], s["Epnb"], v, Ev) + loc
                        s["pnb"] = new
                    continue
                f = lm_term(alpha, l, beta, dtype, mutate)
                g2 = dtype(b["g"] + f)
                Eg2 = b["Eg"] + (1 + SLACK) * U * (abs(float(f)) + abs(float(g2)))
                ctx2 = b["ctx"] if mutate == "ctx_fixed" else (b["ctx"] * V + c) % mod
                cands.append(dict(index=K + k * V + c, seq=target, pb=dtype(NEG), Epb=0.0, pnb=v, Epnb=Ev, g=g2, Eg=Eg2,
                                  ctx=ctx2, score=v, Es=Ev))
        for s in stay:
            s["score"], loc = R.lse2(s["pb"], s["pnb"], dtype)
            s["Es"] = R._pred(s["pb"], s["Epb"], s["pnb"], s["Epnb"]) + loc
        cands = [x for x in stay + cands if x["score"] > NEG]
        for x in cands:
            x["rank"] = dtype(x["score"] + x["g"])
            x["E"] = x["Es"] + x["Eg"] + (1 + SLACK) * U * abs(float(x["rank"]))
        cands.sort(key=lambda x: (-float(x["rank"]), x["index"]))
        for i in range(min(K, len(cands) - 1)):
            gap, both = float(cands[i]["rank"]) - float(cands[i + 1]["rank"]), cands[i]["E"] + cands[i + 1]["E"]
            margin = gap / both if both > 0 else (math.inf if gap > 0 else 0.0)
            min_margin = min(min_margin, margin)
            decided = decided and margin > 1.0
        beams = cands[:K]
    out = {k: [] for k in ("scores", "ctc_scores", "lm_scores", "bounds", "ctc_bounds", "lm_bounds")}
    for b in beams:
        s, loc = R.lse2(b["pb"], b["pnb"], dtype)
        Es = R._pred(b["pb"], b["Epb"], b["pnb"], b["Epnb"]) + loc
        rank = dtype(s + b["g"])
        for k, v in (("scores", rank), ("ctc_scores", s), ("lm_scores", b["g"]), ("ctc_bounds", Es), ("lm_bounds", b["Eg"]),
                     ("bounds", Es + b["Eg"] + (1 + SLACK) * U * abs(float(rank)))):
            out[k].append(float(v))
    out = {k: np.array(v) for k, v in out.items()}
    out.update(tokens=[b["seq"] for b in beams], lengths=[len(b["seq"]) for b in beams], n_beams=len(beams), decided=decided,
               min_margin=min_margin, n_merges=n_merges, n_forbidden=int(n_forbidden))
    return out


def g_along(seq, lm, order, alpha, beta, V, blank=0):
    """g of a token sequence as the device computes it: fp32, one fma and one add per token, in token order."""
    lm = np.asarray(lm, dtype=np.float64).reshape(-1, V)
    g, ctx, mod = np.float32(0.0), start_ctx(V, order, blank), V ** (order - 1)
    for c in seq:
        g = np.float32(g + fma32(np.float32(alpha), lm[ctx, c], np.float32(beta)))
        ctx = (ctx * V + c) % mod
    return g


def differs(got, ref):
    """Would the checks of the exact tier fail?  Tokens, lengths, n_beams equal; each of the three scores within its bound."""
    if got["tokens"] != ref["tokens"] or got["n_beams"] != ref["n_beams"]:
        return True
    return any(bool((np.abs(got[s] - ref[s]) > ref[b]).any())
               for s, b in (("scores", "bounds"), ("ctc_scores", "ctc_bounds"), ("lm_scores", "lm_bounds")))


# ===================================================================================================== inputs
ALPHA, BETA = 0.5, 0.25


def lm_table(V, order, seed, neginf=0.0):
    """fp32-exact float64 [V^(order-1), V]: normal logits x 2, log-softmax per row, rounded to fp32; ``neginf``: that share
    of the entries -inf (chosen after the softmax, so the other entries do not move)."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((V ** (order - 1), V)) * 2.0
    x = (x - np.logaddexp.reduce(x, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    if neginf > 0:
        x[g.random(x.shape) < neginf] = NEG
    return x


# the seeds of the tables: 7 + order, others where a search for decided inputs (never the bound) chose them
LM_SEEDS = {("V64 K8 T40", 1): 15}


def lm_seed(name, order):
    return LM_SEEDS.get((name, order), 7 + order)


# (name, beam case, order, table seed, share of -inf entries, blank): every EXACT_CASE of _ctc_beam_ref at order 1, 2, 3 ...
LM_CASES = [(f"{c[0]} o{order}", c, order, lm_seed(c[0], order), 0.0, 0) for c in R.EXACT_CASES for order in (1, 2, 3)]
# ... two tables with about 10 % forbidden transitions, and order 4 at V 8 with the blank in the last column (the start
# context is then not row 0)
LM_CASES += [
    ("V32 K4 T100 o2 neginf", ("V32 K4 T100", "peaky", 32, 4, 100, 1, 8.0), 2, 21, 0.1, 0),
    ("V3 K8 T16 o3 neginf", ("V3 K8 T16", "peaky", 3, 8, 16, 1, 4.0), 3, 22, 0.1, 0),
    ("V8 K4 T48 o4 blank7", ("V8 K4 T48", "peaky", 8, 4, 48, 3, 6.0), 4, 23, 0.0, 7),
]


def case_inputs(case):
    """-> (lp, lm, K, T, V, order, blank).  With the blank in column b the log-probs of the beam case are rotated so that its
    blank column comes to b."""
    name, bc, order, seed, neginf, blank = case
    lp = R.case_lp(bc)
    V = bc[2]
    if blank:
        lp = np.roll(lp, blank, axis=1)
    return lp, lm_table(V, order, seed, neginf), bc[3], bc[4], V, order, blank


_REF = {}


def case_ref(case):
    """(inputs, the float64 reference) of a case, computed once per process and left unchanged."""
    if case[0] not in _REF:
        inp = case_inputs(case)
        lp, lm, K, T, V, order, blank = inp
        _REF[case[0]] = (inp, beam_lm_ref(lp, K, lm, order, ALPHA, BETA, T=T, blank=blank))
    return _REF[case[0]]
