"""Float64 references, seeded inputs and bounds for the CTC kernels (csrc/ctc.hip): tmi_ctc_logsoftmax, tmi_ctc_greedy,
tmi_ctc_forward and tmi_ctc_viterbi, written literally from the definitions in include/tethys_mi.h.  CPU only: nothing
here imports the GPU package, so tests/test_ctc_cpu.py checks the references (against torch's ctc_loss in float64 and a
brute force over all paths) and the bounds (reachable by an honest fp32 transcription, exceeded by every listed mutation)
before tests/test_wav2vec2_ctc_kernels_gpu.py and tests/test_ctc_gpu.py compare a kernel with them.

The bounds are derived, not fitted.  U = 2^-24 is the unit roundoff of an fp32 add; gam(n) = n U / (1 - n U) bounds a chain
of n roundings.  The device's exp and log are the ROCm device library's expf / logf.  No accuracy table of that library
is installed beside the compiler here, so this is stated as an ASSUMPTION: the library is built to the OpenCL C accuracy
requirements, which allow 3 ulp for exp and 3 ulp for log in fp32 (EXP_ULPS, LOG_ULPS; an ulp is at most 2^-23 of the
value).  numpy's fp32 exp / log are well inside that.

The bound of the forward recursion.  LSE is non-expansive in the sup norm - |LSE(a') - LSE(a)| <= max_i |a'_i - a_i| - so
with E_t(s) a bound on the error of the device's alpha_t(s),
    E_t(s) <= max over the PRESENT, finite predecessors of E_{t-1}  +  loc_t(s)
and loc_t(s) collects what step t itself rounds, every magnitude taken from the float64 reference:
    d_i = a_i - m          one rounding of a value in [-inf, 0]: exp(d_i (1 + U)) is off by the factor exp(d_i U), and
                           |d| exp(d) <= 1 / e, so each of the three terms moves the sum (>= 1) by at most U / e
    e_i = exp(d_i)         EXP_ULPS ulps each: relative C_EXP on the sum
    (e0 + e1) + e2         two adds: 2 U relative
    log(sum)               a relative error r of the sum is an absolute error <= r (1 + r) of the log, plus LOG_ULPS ulps of
                           log(sum) <= log 3 itself
    m + log(sum)           one add: U |lse|
    lp + lse               one add: U |alpha_t(s)|
(1 + SLACK) covers the second-order terms and the difference between the device's magnitudes and the reference's.  A state
with one finite predecessor computes exp(0) = 1 and log(1) = 0 exactly; it is charged the same.  The final
-LSE(alpha(S-1), alpha(S-2)) is one more such step with two terms and no lp.  The bound is carried per state next to the
recursion (``ctc_forward_ref``) and returned per item.
"""
import itertools
import math

import numpy as np
import torch

U = 2.0 ** -24
EXP_ULPS, LOG_ULPS = 3, 3
C_EXP, C_LOG = EXP_ULPS * 2.0 ** -23, LOG_ULPS * 2.0 ** -23
SLACK = 2.0 ** -10
NEG = -np.inf
F32, I32 = torch.float32, torch.int32
V_DEFAULT = 32


def gam(n):
    return n * U / (1.0 - n * U)


def guard_pattern(n, dtype):
    """7.0 / NaN alternating (integers: 7 / a large negative): a stray store of any finite value, or of NaN, shows."""
    t = torch.full((n,), 7, dtype=dtype)
    t[1::2] = float("nan") if dtype.is_floating_point else -(2 ** 30)
    return t


def ratio(got, ref, bound):
    """max over elements of |got - ref| / bound.  An element equal to its reference (equal infinities included) counts 0
    whatever its bound; a NaN, a wrong infinity or an error against a zero bound counts inf."""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64).reshape(-1) if np.ndim(bound) else np.float64(bound), ref.shape)
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - ref) / bound
    r = np.where(got == ref, 0.0, r)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


# ===================================================================================================== inputs
def logits_inputs(R, V, seed, scale=1.5):
    """fp32-exact logits as float64 [R, V]."""
    g = np.random.default_rng(seed)
    return (g.standard_normal((R, V)) * scale).astype(np.float32).astype(np.float64)


def lp_inputs(T, V, seed, scale=1.5):
    """fp32-exact log-probabilities as float64 [T, V]: the log-softmax of random logits, rounded to fp32."""
    x = logits_inputs(T, V, seed, scale)
    return logsoftmax_ref(x)[0].astype(np.float32).astype(np.float64)


def grid_lp(T, V, seed, step=64, span=1024):
    """Values k / step, |k| <= span: every fp32 sum of up to 4096 of them is exact (|sum| * 64 < 2^24)."""
    g = np.random.default_rng(seed)
    return g.integers(-span, span + 1, size=(T, V)).astype(np.float64) / step


def labels_for(kind, L, V, seed, blank=0):
    """'random': any non-blank symbol; 'equal': one symbol throughout; 'alt': two symbols alternating; 'distinct': no two
    neighbours equal."""
    g = np.random.default_rng(seed)
    syms = np.array([v for v in range(V) if v != blank])
    if kind == "equal":
        return np.full(L, syms[3 % len(syms)], dtype=np.int64)
    if kind == "alt":
        return np.where(np.arange(L) % 2 == 0, syms[1], syms[2]).astype(np.int64)
    lab = syms[g.integers(0, len(syms), size=L)].astype(np.int64)
    if kind == "distinct":
        for i in range(1, L):
            while lab[i] == lab[i - 1]:
                lab[i] = syms[g.integers(0, len(syms))]
    return lab


def min_frames(labels):
    """The fewest frames that carry the labels: one each, and a blank between equal neighbours."""
    labels = np.asarray(labels)
    return int(len(labels) + (labels[1:] == labels[:-1]).sum())


# ============================================================================================== log-softmax
def logsoftmax_ref(x):
    """x float64 [R, V] -> (logp float64, argmax int64 (the smallest column among equal maxima), bound [R, V]).
    Bound per element, for the wave form of csrc/ctc.hip: V terms exp(x - m) (argument rounding U / e each against a sum
    >= 1, C_EXP relative), a butterfly of 6 adds (gam(6) relative), the log (C_LOG of |log s|), m + log s (U |lse|) and
    x - lse (U |logp|)."""
    x = np.asarray(x, dtype=np.float64)
    R, V = x.shape
    m = x.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.exp(x - m).sum(axis=1, keepdims=True)
        lse = m + np.log(s)
        logp = x - lse
        rs = C_EXP + V * U / math.e + gam(6)
        bound = (1 + SLACK) * (rs * (1 + rs) + C_LOG * np.abs(np.log(s)) + U * np.abs(lse) + U * np.abs(logp))
    bound = np.where(np.isfinite(logp), bound, 0.0)
    return logp, np.argmax(x, axis=1), bound


# =================================================================================================== greedy
GREEDY_THREADS = 256


def greedy_ref(argmax, logp, length, blank):
    """argmax int [T], logp float64 [T, V] -> dict(tokens, start, end, best, best_bound).  The bound of best: a term
    passes through at most ceil(len / 256) adds on its thread, 6 in the wave butterfly and 3 over the waves."""
    a = np.asarray(argmax)[:length]
    tokens, start, end = [], [], []
    for t in range(length):
        if a[t] != blank and (t == 0 or a[t] != a[t - 1]):
            tokens.append(int(a[t]))
            start.append(t)
            e = t
            while e + 1 < length and a[e + 1] == a[t]:
                e += 1
            end.append(e + 1)
    terms = np.asarray(logp, dtype=np.float64)[np.arange(length), a]
    depth = -(-length // GREEDY_THREADS) + 9
    return {"tokens": np.array(tokens, dtype=np.int64), "start": np.array(start, dtype=np.int64),
            "end": np.array(end, dtype=np.int64), "best": float(terms.sum()),
            "best_bound": gam(depth) * float(np.abs(terms).sum())}


def greedy_best_f32(argmax, logp, length):
    """The kernel's own order in fp32 numpy (an honest transcription for the CPU test of the bound)."""
    a = np.asarray(argmax)[:length]
    terms = np.asarray(logp, dtype=np.float64)[np.arange(length), a].astype(np.float32)
    acc = np.zeros(GREEDY_THREADS, dtype=np.float32)
    for t0 in range(0, length, GREEDY_THREADS):
        chunk = terms[t0:t0 + GREEDY_THREADS]
        acc[:len(chunk)] += chunk
    w = acc.reshape(4, 64).copy()
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, np.arange(64) ^ o]
    return float(((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])


# ================================================================================= forward recursion and Viterbi
def _ext(labels, blank):
    labels = np.asarray(labels, dtype=np.int64)
    S = 2 * len(labels) + 1
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = labels
    return ext, S


def _skip(ext, blank, mutate):
    S = len(ext)
    skip = np.zeros(S, dtype=bool)
    if S > 2:
        skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
        if mutate == "skip_equal":
            skip[2:] = ext[2:] != blank
        if mutate == "skip_blank":
            skip[2:] = (ext[2:] == blank) | (ext[2:] != ext[:-2])
    return skip


def _shift(a, k, dtype):
    out = np.full(len(a), NEG, dtype=dtype)
    if len(a) > k:
        out[k:] = a[:len(a) - k]
    return out


def _lse(terms, dtype):
    """LSE over axis 0 in ``dtype``, in the kernel's order; all -inf -> -inf.  -> (lse, the sum of exponentials)."""
    m = terms[0]
    for t in terms[1:]:
        m = np.maximum(m, t)
    dead = m == NEG
    ms = np.where(dead, dtype(0), m).astype(dtype)
    s = np.exp((terms[0] - ms).astype(dtype)).astype(dtype)
    for t in terms[1:]:
        s = (s + np.exp((t - ms).astype(dtype)).astype(dtype)).astype(dtype)
    with np.errstate(divide="ignore"):
        out = (ms + np.log(s).astype(dtype)).astype(dtype)
    return np.where(dead, dtype(NEG), out).astype(dtype), s


def ctc_forward_ref(lp, labels, T=None, blank=0, dtype=np.float64, mutate=None):
    """lp float64 [>= T, V] (fp32-exact), labels int [L] -> dict(nll, infeasible, bound).  ``dtype=np.float32`` is the honest
    fp32 transcription.  ``mutate``: None, or one of MUTATIONS (a deliberately wrong recursion, for the test of the bound).
    T < 1 is infeasible."""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0] if T is None else T
    if mutate == "frame_more":
        T += 1
    if mutate == "frame_less":
        T -= 1
    ext, S = _ext(labels, blank)
    if T < 1:
        return {"nll": math.inf, "infeasible": 1, "bound": 0.0}
    skip = _skip(ext, blank, mutate)
    lpe = lp[:T][:, ext].astype(dtype)                    # [T, S]: the column each state reads
    alpha = np.full(S, NEG, dtype=dtype)
    alpha[:2] = lpe[0, :2]
    E = np.zeros(S)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(1, T):
            a0, a1 = alpha, _shift(alpha, 1, dtype)
            a2 = np.where(skip, _shift(alpha, 2, dtype), dtype(NEG)).astype(dtype)
            if mutate == "max":
                lse, s = np.maximum(a0, np.maximum(a1, a2)), np.ones(S)
            else:
                lse, s = _lse([a0, a1, a2], dtype)
            new = (lpe[t] + lse).astype(dtype)
            if dtype is np.float64:
                e1, e2 = _shift(E, 1, np.float64), _shift(E, 2, np.float64)
                pred = np.maximum(np.where(np.isfinite(a0), E, 0.0),
                                  np.maximum(np.where(np.isfinite(a1), np.nan_to_num(e1, neginf=0.0), 0.0),
                                             np.where(np.isfinite(a2), np.nan_to_num(e2, neginf=0.0), 0.0)))
                rs = C_EXP + 3 * U / math.e + 2 * U
                loc = (1 + SLACK) * (rs * (1 + rs) + C_LOG * np.abs(np.log(np.maximum(s, 1.0)))
                                     + U * np.abs(np.nan_to_num(lse, neginf=0.0)) + U * np.abs(np.nan_to_num(new, neginf=0.0)))
                E = np.where(np.isfinite(new), pred + loc, 0.0)
            alpha = new
        last = alpha[S - 1]
        prev = alpha[S - 2] if S > 1 else dtype(NEG)
        if mutate == "final_one":
            prev = dtype(NEG)
        ll, s = _lse([np.array([last], dtype=dtype), np.array([prev], dtype=dtype)], dtype)
    ll = float(ll[0])
    if ll == NEG:
        return {"nll": math.inf, "infeasible": 1, "bound": 0.0}
    pred = max(E[S - 1] if np.isfinite(last) else 0.0, (E[S - 2] if S > 1 and np.isfinite(prev) else 0.0))
    rs = C_EXP + 2 * U / math.e + U
    bound = pred + (1 + SLACK) * (rs * (1 + rs) + C_LOG * abs(math.log(max(float(s[0]), 1.0))) + U * abs(ll))
    return {"nll": -ll, "infeasible": 0, "bound": float(bound)}


MUTATIONS = ["skip_equal", "skip_blank", "final_one", "frame_more", "frame_less", "max"]


def viterbi_ref(lp, labels, T=None, blank=0, dtype=np.float64, ties="first"):
    """The max semiring with the tie rule of include/tethys_mi.h -> dict(total, infeasible, states [T], start [L], end [L]).
    ``ties="last"`` is the mutation that resolves every tie the other way."""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0] if T is None else T
    ext, S = _ext(labels, blank)
    L = len(labels)
    none = {"total": -math.inf, "infeasible": 1, "states": np.full(max(T, 0), -1, dtype=np.int64),
            "start": np.full(L, -1, dtype=np.int64), "end": np.full(L, -1, dtype=np.int64)}
    if T < 1:
        return none
    skip = _skip(ext, blank, None)
    lpe = lp[:T][:, ext].astype(dtype)
    alpha = np.full(S, NEG, dtype=dtype)
    alpha[:2] = lpe[0, :2]
    moves = np.zeros((T, S), dtype=np.int64)
    gt = (lambda a, b: a > b) if ties == "first" else (lambda a, b: a >= b)
    for t in range(1, T):
        a1 = _shift(alpha, 1, dtype)
        a2 = np.where(skip, _shift(alpha, 2, dtype), dtype(NEG)).astype(dtype)
        best, mv = alpha.copy(), np.zeros(S, dtype=np.int64)
        w = gt(a1, best)
        best, mv = np.where(w, a1, best), np.where(w, 1, mv)
        w = gt(a2, best) & skip
        best, mv = np.where(w, a2, best), np.where(w, 2, mv)
        alpha = (lpe[t] + best).astype(dtype)
        moves[t] = mv
    s = S - 1
    if S > 1 and (alpha[S - 2] > alpha[S - 1] if ties == "first" else alpha[S - 2] >= alpha[S - 1]):
        s = S - 2
    total = float(alpha[s])
    if total == NEG:
        return none
    states = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        if t > 0:
            s -= min(int(moves[t, s]), s)
    start, end = np.full(L, -1, dtype=np.int64), np.full(L, -1, dtype=np.int64)
    for i in range(L):
        at = np.nonzero(states == 2 * i + 1)[0]
        if len(at):
            start[i], end[i] = at[0], at[-1] + 1
    return {"total": total, "infeasible": 0, "states": states, "start": start, "end": end}


def path_problems(states, labels, T, start=None, end=None, blank=0):
    """What is wrong with a path of extended states (an empty list: a valid CTC path)."""
    ext, S = _ext(labels, blank)
    st = np.asarray(states)[:T]
    bad = []
    if len(st) != T or (st < 0).any() or (st >= S).any():
        return ["states outside [0, S)"]
    if st[0] > 1:
        bad.append("starts past state 1")
    if st[-1] < S - 2:
        bad.append("ends before state S-2")
    d = np.diff(st)
    if ((d < 0) | (d > 2)).any():
        bad.append("not monotone or a step wider than 2")
    for t in np.nonzero(d == 2)[0]:
        s = st[t + 1]
        if s % 2 == 0 or ext[s] == ext[s - 2]:
            bad.append(f"illegal skip into state {s}")
    if start is not None:
        for i in range(len(labels)):
            at = np.nonzero(st == 2 * i + 1)[0]
            if len(at) == 0 or start[i] != at[0] or end[i] != at[-1] + 1:
                bad.append(f"bounds of token {i}")
    return bad


def path_score(lp, labels, states, blank=0):
    ext, _ = _ext(labels, blank)
    st = np.asarray(states)
    return float(np.asarray(lp, dtype=np.float64)[np.arange(len(st)), ext[st]].sum())


def path_bound(lp, labels, states, blank=0):
    """e(P): the rounding of the fp32 running sum along a path, gam(T - 1) sum |lp|."""
    ext, _ = _ext(labels, blank)
    st = np.asarray(states)
    return gam(max(len(st) - 1, 1)) * float(np.abs(np.asarray(lp, dtype=np.float64)[np.arange(len(st)), ext[st]]).sum())


def viterbi_brute(lp, labels, blank=0):
    """The maximum over ALL valid paths by enumeration (T <= 6, L <= 2)."""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0]
    ext, S = _ext(labels, blank)
    best = -math.inf
    for st in itertools.product(range(S), repeat=T):
        if path_problems(np.array(st), labels, T, blank=blank) == []:
            best = max(best, path_score(lp, labels, st, blank))
    return best


# ============================================================================================== shape classes
# (name, T, L, label kind): the classes of the issue at V = 32 - the wave seams sit at S = 63 / 65 (L 31 / 32) and
# 255 / 257 (L 127 / 128); "exact" / "short": exactly enough frames and one too few.
def forward_cases():
    cases = []
    for L in (0, 1, 2, 31, 32, 33, 127, 128):
        cases.append((f"T300 L{L}", 300, L, "random"))
    cases.append(("T600 L511", 600, 511, "random"))
    cases += [("T1 L0", 1, 0, "random"), ("T1 L1", 1, 1, "random"), ("T1 L2 infeasible", 1, 2, "distinct"),
              ("T2 L1", 2, 1, "random"), ("T2 L2 exact", 2, 2, "distinct"), ("T2 L2 equal infeasible", 2, 2, "equal"),
              ("T65 L31", 65, 31, "random"), ("T65 L32", 65, 32, "distinct"),
              ("T65 L20 equal", 65, 20, "equal"), ("T39 L20 equal exact", 39, 20, "equal"),
              ("T38 L20 equal short", 38, 20, "equal"), ("T300 L33 alt", 300, 33, "alt")]
    lab = labels_for("random", 33, V_DEFAULT, 733)
    cases.append(("L33 exact", min_frames(lab), 33, "random"))
    cases.append(("L33 short", min_frames(lab) - 1, 33, "random"))
    return cases


def case_inputs(case, V=V_DEFAULT):
    """-> (lp float64 [T + 1, V] (one spare frame, for the frame_more mutation), labels int64 [L], T)."""
    name, T, L, kind = case
    seed = 733 if name.startswith("L33") else (sum(map(ord, name)) * 31 + T)
    return lp_inputs(T + 1, V, seed + 1), labels_for(kind, L, V, seed), T


def torch_ctc(lp, labels, T, blank=0):
    """torch.nn.functional.ctc_loss in float64 on the CPU, one item, reduction none."""
    lpt = torch.from_numpy(np.asarray(lp, dtype=np.float64)[:T]).unsqueeze(1)
    tg = torch.from_numpy(np.asarray(labels, dtype=np.int64)).unsqueeze(0)
    out = torch.nn.functional.ctc_loss(lpt, tg, torch.tensor([T]), torch.tensor([len(labels)]), blank=blank, reduction="none")
    return float(out[0])


def levenshtein(hyp, ref):
    """Edit distance of two integer sequences (plain dynamic program; the model's own is row-vectorised)."""
    d = list(range(len(ref) + 1))
    for i, h in enumerate(hyp, 1):
        prev, d[0] = d[0], i
        for j, r in enumerate(ref, 1):
            prev, d[j] = d[j], min(d[j] + 1, d[j - 1] + 1, prev + (h != r))
    return d[len(ref)]
