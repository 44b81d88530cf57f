"""Float64 reference, brute force, seeded cases and bounds for tmi_ctc_posteriors (csrc/ctc_post.hip), written literally
from the definitions in include/tethys_mi.h.  CPU only: nothing here imports the GPU package, so
tests/test_ctc_post_cpu.py checks the reference (against a brute force over all paths, finite differences of
``_ctc_ref.ctc_forward_ref`` and torch's float64 ctc_loss) and the bounds (reachable by an honest fp32 transcription,
exceeded by every listed mutation) before tests/test_ctc_post_kernels_gpu.py and tests/test_ctc_post_gpu.py compare a
kernel with them.

The definitions (ext = [blank, l1, blank, .., lL, blank], S = 2L + 1, lp = the item's log-probs, LSE3 the LSE of
tmi_ctc_forward):
    alpha:  alpha_t(s) is the recursion of tmi_ctc_forward, in the same operation order.  ll = -(the unclamped nll).
    beta:   beta_{T-1}(s) = lp[T-1][ext_s] for s = S-1 and, if S > 1, s = S-2; -inf elsewhere.
            beta_t(s) = lp[t][ext_s] + LSE3(beta_{t+1}(s), beta_{t+1}(s+1), beta_{t+1}(s+2)).
            The second term applies only if s+1 < S.
            The third term applies only if s+2 < S && ext_{s+2} != blank && ext_{s+2} != ext_s.
    gamma:  gamma[n,t,s] = exp((alpha_t(s) - ll) + (beta_t(s) - lp[t][ext_s])): the two differences first, then their sum.
            It is 0 whenever alpha_t(s) or beta_t(s) is -inf.  gamma is not clamped to 1.
    occ:    occ[n,t,c] = sum over s ascending with ext_s == c of gamma[n,t,s], a running sum from 0.
    grad:   grad[n,t,c] = expf(lp[t][c]) - occ[n,t,c].
    tok_frames:  tok_frames[n,i] = sum over t of gamma[n,t,2i+1], a running sum from 0 in descending t.
    tok_center:  tok_center[n,i] = (sum over t of t * gamma[n,t,2i+1]) / tok_frames[n,i].  The product t * gamma is formed
            with t converted to fp32 and rounded before it is added.  The sum takes the same order as tok_frames.

The bounds are derived, not fitted, from the constants of ``_ctc_ref`` (U, gam, EXP_ULPS, LOG_ULPS, SLACK; its docstring
states the assumption on the device's expf / logf).
    alpha   E_a, carried per state exactly as ``ctc_forward_ref`` carries it: the largest bound of a present, finite
            predecessor plus what the step rounds.
    beta    E_b, the mirror: the predecessors are states s, s+1, s+2 of frame t+1.
    ll      E_ll, the nll bound of ``ctc_forward_ref``.
    gamma   the exponent x = (alpha - ll) + (beta - lp) carries Ex = E_a + E_b + E_ll + U (|alpha - ll| + |beta - lp| + |x|)
            (lp is an exact input); through exp, |gamma' - gamma| <= gamma (e^Ex - 1) + EXP_ULPS ulps of gamma e^Ex, plus
            TINY = 2^-126, the smallest normal fp32: below it a device may round to a denormal or flush to zero.
    occ     the bounds of its count terms, plus gam(count) of the terms (the running sum).
    grad    that, plus EXP_ULPS ulps of exp(lp) and U |grad| for the subtraction, plus TINY: exp(lp) of a log-prob below
            -87.3 lies under the smallest normal as well.
    tok_frames  the bounds of its T terms plus gam(T) of the terms.
    tok_center  numerator: t times each term's bound, U per product, gam(T) of the terms; the quotient of two such sums
            moves by (b_num + center b_den) / (den - b_den), and the division itself rounds once more (2 U |center|).
This worst case is loose for long clips (every frame step is charged its full rounding, about 1.3e-6, and gamma sees the
accumulated alpha and beta bounds through exp): ``bound_report`` prints what it is at each shape.  Accuracy is therefore
told at the short shapes, where it is tight; the long shapes are held to the same bound AND to what the contract states
exactly at any length (nll and the flags bit for bit tmi_ctc_forward's, the untouched regions, the same bits twice, with and
without grad, alone and in a batch)."""
import math

import numpy as np
import torch

import _ctc_ref as C

U, SLACK, C_EXP, C_LOG, NEG, gam = C.U, C.SLACK, C.C_EXP, C.C_LOG, C.NEG, C.gam
TINY = 2.0 ** -126
KEYS = ("gamma", "occ", "grad", "tok_frames", "tok_center")

MUTATIONS = ["beta_skip_back",    # the beta skip rule tested on ext_s vs ext_{s-2} instead of ext_{s+2} vs ext_s
             "beta_skip_equal",   # the skip allowed across equal labels
             "beta_init_one",     # beta_{T-1}(S-2) left out
             "lp_twice",          # lp counted twice in gamma: exp(alpha + beta - ll)
             "occ_parity",        # occ folded by state parity (even: the blank, odd: the first label) instead of by symbol
             "grad_sign",         # occ - exp(lp)
             "beta_frame_less"]   # the beta pass starts one frame early: frame T-1 gets no beta


def _shift_dn(a, k, dtype):
    out = np.full(len(a), NEG, dtype=dtype)
    if len(a) > k:
        out[:len(a) - k] = a[k:]
    return out


def _loc(s, lse, new):
    """What one frame step rounds (the docstring of _ctc_ref), magnitudes from the float64 values."""
    rs = C_EXP + 3 * U / math.e + 2 * U
    return (1 + SLACK) * (rs * (1 + rs) + C_LOG * np.abs(np.log(np.maximum(s, 1.0)))
                          + U * np.abs(np.nan_to_num(lse, neginf=0.0)) + U * np.abs(np.nan_to_num(new, neginf=0.0)))


def _pred(vals, Es):
    out = np.zeros(len(vals[0]))
    for v, e in zip(vals, Es):
        out = np.maximum(out, np.where(np.isfinite(v), np.nan_to_num(e, neginf=0.0), 0.0))
    return out


def _none(T, S, L, V):
    T = max(T, 0)
    z = {"nll": math.inf, "ll": NEG, "infeasible": 1, "bound_nll": 0.0, "gamma": np.zeros((T, S)), "occ": np.zeros((T, V)),
         "grad": np.zeros((T, V)), "tok_frames": np.zeros(L), "tok_center": np.full(L, -1.0)}
    z.update({"b_" + k: np.zeros_like(z[k]) for k in KEYS})
    return z


def post_ref(lp, labels, T=None, blank=0, dtype=np.float64, mutate=None):
    """lp float64 [>= T, V] (fp32-exact), labels int [L] -> dict(nll, ll, infeasible, bound_nll, gamma [T, S], occ [T, V],
    grad [T, V], tok_frames [L], tok_center [L], and with float64 ``b_<name>``: the bound of each, element for element).
    ``dtype=np.float32`` is the honest transcription of the device's order; ``mutate``: None or one of MUTATIONS.  A label
    outside [0, V) has log-prob -inf.  T < 1, or no finite path: zeros, tok_center -1, every bound 0."""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0] if T is None else T
    V = lp.shape[1]
    labels = np.asarray(labels, dtype=np.int64)
    L = len(labels)
    ext, S = C._ext(labels, blank)
    if T < 1:
        return _none(T, S, L, V)
    f64 = dtype is np.float64
    valid = (ext >= 0) & (ext < V)
    lpe = np.where(valid[None, :], lp[:T][:, np.where(valid, ext, 0)], NEG).astype(dtype)   # [T, S]: the column each state reads
    skip = C._skip(ext, blank, None)
    skipb = np.zeros(S, dtype=bool)
    if S > 2:
        skipb[:S - 2] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
        if mutate == "beta_skip_equal":
            skipb[:S - 2] = ext[2:] != blank
        if mutate == "beta_skip_back":
            back = np.ones(S, dtype=bool)
            back[2:] = ext[2:] != ext[:-2]
            skipb[:S - 2] = ((ext != blank) & back)[:S - 2]
    A, B = np.full((T, S), NEG, dtype=dtype), np.full((T, S), NEG, dtype=dtype)
    EA, EB = np.zeros((T, S)), np.zeros((T, S))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        # ---- alpha: ctc_forward_ref's loop, every frame kept
        A[0, :2] = lpe[0, :2]
        for t in range(1, T):
            a0, a1 = A[t - 1], C._shift(A[t - 1], 1, dtype)
            a2 = np.where(skip, C._shift(A[t - 1], 2, dtype), dtype(NEG)).astype(dtype)
            lse, s = C._lse([a0, a1, a2], dtype)
            A[t] = (lpe[t] + lse).astype(dtype)
            if f64:
                pred = _pred([a0, a1, a2], [EA[t - 1], C._shift(EA[t - 1], 1, np.float64), C._shift(EA[t - 1], 2, np.float64)])
                EA[t] = np.where(np.isfinite(A[t]), pred + _loc(s, lse, A[t]), 0.0)
        last = A[T - 1, S - 1]
        prev = A[T - 1, S - 2] if S > 1 else dtype(NEG)
        llv, s = C._lse([np.array([last], dtype=dtype), np.array([prev], dtype=dtype)], dtype)
        ll = dtype(llv[0])
        if ll == NEG:
            return _none(T, S, L, V)
        pred = max(EA[T - 1, S - 1] if np.isfinite(last) else 0.0, EA[T - 1, S - 2] if S > 1 and np.isfinite(prev) else 0.0)
        rs = C_EXP + 2 * U / math.e + U
        E_ll = pred + (1 + SLACK) * (rs * (1 + rs) + C_LOG * abs(math.log(max(float(s[0]), 1.0))) + U * abs(float(ll)))
        # ---- beta: the mirror
        t_last = T - 2 if mutate == "beta_frame_less" else T - 1
        if t_last >= 0:
            B[t_last, S - 1] = lpe[t_last, S - 1]
            if S > 1 and mutate != "beta_init_one":
                B[t_last, S - 2] = lpe[t_last, S - 2]
        for t in range(t_last - 1, -1, -1):
            b0, b1 = B[t + 1], _shift_dn(B[t + 1], 1, dtype)
            b2 = np.where(skipb, _shift_dn(B[t + 1], 2, dtype), dtype(NEG)).astype(dtype)
            lse, s = C._lse([b0, b1, b2], dtype)
            B[t] = (lpe[t] + lse).astype(dtype)
            if f64:
                pred = _pred([b0, b1, b2], [EB[t + 1], _shift_dn(EB[t + 1], 1, np.float64), _shift_dn(EB[t + 1], 2, np.float64)])
                EB[t] = np.where(np.isfinite(B[t]), pred + _loc(s, lse, B[t]), 0.0)
        # ---- gamma
        live = np.isfinite(A) & np.isfinite(B)
        d1 = np.where(live, (A - ll).astype(dtype), dtype(0)).astype(dtype)
        d2 = np.where(live, (B - lpe).astype(dtype), dtype(0)).astype(dtype)
        if mutate == "lp_twice":
            d2 = np.where(live, B, dtype(0)).astype(dtype)
        x = (d1 + d2).astype(dtype)
        gamma = np.where(live, np.exp(x).astype(dtype), dtype(0)).astype(dtype)
        bg = np.zeros((T, S))
        if f64:
            Ex = EA + EB + E_ll + (1 + SLACK) * U * (np.abs(d1) + np.abs(d2) + np.abs(x))
            bg = np.where(live, (1 + SLACK) * gamma * (np.expm1(Ex) + C_EXP * np.exp(Ex)) + TINY, 0.0)
        # ---- occ, s ascending
        occ, b_occ, cnt, mag = np.zeros((T, V), dtype=dtype), np.zeros((T, V)), np.zeros(V), np.zeros((T, V))
        for si in range(S):
            c = ext[si]
            if mutate == "occ_parity":
                c = blank if si % 2 == 0 else ext[1]
            if not 0 <= c < V:
                continue
            occ[:, c] = (occ[:, c] + gamma[:, si]).astype(dtype)
            b_occ[:, c] += bg[:, si]
            mag[:, c] += gamma[:, si] + bg[:, si]
            cnt[c] += 1
        b_occ = b_occ + gam(cnt)[None, :] * mag
        p = np.exp(lp[:T].astype(dtype)).astype(dtype)
        grad = (occ - p).astype(dtype) if mutate == "grad_sign" else (p - occ).astype(dtype)
        b_grad = (1 + SLACK) * (b_occ + C_EXP * np.exp(lp[:T]) + U * np.abs(grad.astype(np.float64))) + TINY
        # ---- token sums, t descending
        tf, tc = np.zeros(L, dtype=dtype), np.zeros(L, dtype=dtype)
        for t in range(T - 1, -1, -1):
            g = gamma[t, 1::2]
            tf = (tf + g).astype(dtype)
            tc = (tc + (dtype(t) * g).astype(dtype)).astype(dtype)
        center = (tc / np.where(tf > 0, tf, dtype(1))).astype(dtype)
        g64, bgt = gamma[:, 1::2].astype(np.float64), bg[:, 1::2]
        tt = np.arange(T, dtype=np.float64)[:, None]
        b_tf = bgt.sum(0) + gam(T) * (g64 + bgt).sum(0)
        b_num = (tt * bgt).sum(0) + U * (tt * g64).sum(0) + gam(T) * (tt * (g64 + bgt)).sum(0)
        den = np.maximum(tf.astype(np.float64) - b_tf, TINY)
        b_tc = (1 + SLACK) * ((b_num + np.abs(center) * b_tf) / den + 2 * U * np.abs(center))
    return {"nll": -float(ll), "ll": float(ll), "infeasible": 0, "bound_nll": float(E_ll), "gamma": gamma, "occ": occ,
            "grad": grad, "tok_frames": tf, "tok_center": center, "b_gamma": bg, "b_occ": b_occ, "b_grad": b_grad,
            "b_tok_frames": b_tf, "b_tok_center": b_tc, "alpha": A, "beta": B}


def ratios(got, ref):
    """max |got - ref| / bound per output of KEYS, and of the rows of occ summing to 1 (``occ_rows``: the sum of a row's
    bounds, the float64 reference's own rows sum to 1 within 1e-12)."""
    out = {k: C.ratio(got[k], ref[k], ref["b_" + k]) for k in KEYS}
    if not ref["infeasible"] and ref["occ"].shape[0]:
        rows = np.asarray(got["occ"], dtype=np.float64).sum(axis=1)
        out["occ_rows"] = C.ratio(rows, np.ones_like(rows), ref["b_occ"].sum(axis=1) + 1e-12)
    return out


def bound_report(name, ref):
    if ref["infeasible"]:
        return f"{name}: no path"
    return (f"{name}: bounds nll {ref['bound_nll']:.2e}, gamma {ref['b_gamma'].max():.2e}, occ {ref['b_occ'].max():.2e}, "
            f"grad {ref['b_grad'].max():.2e}, tok_frames {ref['b_tok_frames'].max() if len(ref['b_tok_frames']) else 0:.2e}, "
            f"tok_center {ref['b_tok_center'].max() if len(ref['b_tok_center']) else 0:.2e}")


# ============================================================================================== brute force
def _paths(ext, T, blank):
    """Every valid CTC path of T frames over ext, by the transition rules themselves (no recursion over values)."""
    S = len(ext)

    def grow(path):
        if len(path) == T:
            if path[-1] >= S - 2:
                yield tuple(path)
            return
        s = path[-1]
        for d in (0, 1, 2):
            n = s + d
            if n >= S or (d == 2 and (ext[n] == blank or ext[n] == ext[s])):
                continue
            yield from grow(path + [n])
    for s0 in (0, 1):
        if s0 < S:
            yield from grow([s0])


def post_brute(lp, labels, blank=0):
    """gamma, occ, grad, tok_frames, tok_center and nll from the enumeration of all paths (T <= 6, L <= 3)."""
    lp = np.asarray(lp, dtype=np.float64)
    T, V = lp.shape
    ext, S = C._ext(labels, blank)
    L = len(labels)
    gamma, Z = np.zeros((T, S)), 0.0
    for path in _paths(ext, T, blank):
        p = math.exp(sum(lp[t, ext[s]] for t, s in enumerate(path)))
        Z += p
        for t, s in enumerate(path):
            gamma[t, s] += p
    if Z == 0.0:
        return None
    gamma /= Z
    occ = np.zeros((T, V))
    for s in range(S):
        occ[:, ext[s]] += gamma[:, s]
    tf = gamma[:, 1::2].sum(0)
    tc = (np.arange(T)[:, None] * gamma[:, 1::2]).sum(0) / np.where(tf > 0, tf, 1.0)
    return {"nll": -math.log(Z), "gamma": gamma, "occ": occ, "grad": np.exp(lp) - occ, "tok_frames": tf, "tok_center": tc,
            "n_paths": sum(1 for _ in _paths(ext, T, blank))}


def torch_grad(logits, labels, T, blank=0):
    """d ctc_loss(reduction="sum") / d logits through log_softmax, torch CPU float64 -> [T, V]."""
    x = torch.tensor(np.asarray(logits, dtype=np.float64)[:T], requires_grad=True)
    lpt = torch.log_softmax(x, dim=1).unsqueeze(1)
    tg = torch.from_numpy(np.asarray(labels, dtype=np.int64)).unsqueeze(0)
    loss = torch.nn.functional.ctc_loss(lpt, tg, torch.tensor([T]), torch.tensor([len(labels)]), blank=blank, reduction="sum")
    loss.backward()
    return x.grad.numpy()


# ============================================================================================== shape classes
# (name, T, L, label kind, V, flavour).  The wave seams sit at 64 and 128 extended states (L 31 / 32 / 33, 63 / 64), L 127 /
# 128 at 256, L 511 is the 1023-thread case; T 7 / 8 / 9 and 16 / 17 are the edges of the prefetch (CT_PF = 8).  Flavours:
# "" plain; "neginf": -inf entries in lp, never a whole row; "exact": T = min_frames(labels), a single path; "short": one
# frame fewer, no path.  A shape whose labels need more frames than T has no path either: the kernel's zero route at that
# thread count.
def cases():
    out = [("T1 L0", 1, 0, "random", 32, ""), ("T1 L1", 1, 1, "random", 32, ""), ("T1 L31 nopath", 1, 31, "random", 32, ""),
           ("T2 L0", 2, 0, "random", 32, ""), ("T2 L1", 2, 1, "random", 32, ""),
           ("T7 L0", 7, 0, "random", 32, ""), ("T7 L1", 7, 1, "random", 32, ""), ("T7 L3 equal", 7, 3, "equal", 32, ""),
           ("T8 L1", 8, 1, "random", 32, ""), ("T8 L4 alt", 8, 4, "alt", 32, ""),
           ("T9 L1", 9, 1, "random", 32, ""), ("T9 L4 equal", 9, 4, "equal", 32, ""),
           ("T16 L1", 16, 1, "random", 32, ""), ("T16 L5 equal", 16, 5, "equal", 32, ""),
           ("T17 L1", 17, 1, "random", 32, ""), ("T17 L9 alt", 17, 9, "alt", 32, "")]
    for L, kind in ((0, "random"), (1, "random"), (31, "random"), (32, "random"), (33, "alt"), (31, "equal"), (32, "equal"),
                    (33, "equal"), (63, "alt"), (64, "alt"), (127, "random"), (128, "alt"), (511, "random")):
        out.append((f"T64 L{L} {kind}", 64, L, kind, 32, ""))
    out += [("T64 L31 V2", 64, 31, "random", 2, ""), ("T64 L31 V31", 64, 31, "random", 31, ""),
            ("T64 L32 V33", 64, 32, "alt", 33, ""), ("T64 L33 V64", 64, 33, "random", 64, ""),
            ("T17 L5 V2", 17, 5, "random", 2, ""), ("T9 L3 V64", 9, 3, "alt", 64, ""),
            ("T64 L31 neginf", 64, 31, "alt", 32, "neginf"), ("T17 L4 neginf", 17, 4, "random", 32, "neginf"),
            ("L33 exact", 0, 33, "random", 32, "exact"), ("L33 short", 0, 33, "random", 32, "short"),
            ("L20 equal exact", 0, 20, "equal", 32, "exact")]
    return out


def long_cases():
    return [("T1100 L511", 1100, 511, "random", 32, ""), ("T300 L127", 300, 127, "random", 32, ""),
            ("T300 L128 alt", 300, 128, "alt", 32, "")]


def case_inputs(case):
    """-> (lp float64 [T, V] fp32-exact, labels int64 [L], T)."""
    name, T, L, kind, V, flavour = case
    seed = sum(map(ord, name)) * 31 + L
    lab = C.labels_for(kind, L, V, seed)
    if flavour == "exact":
        T = C.min_frames(lab)
    if flavour == "short":
        T = C.min_frames(lab) - 1
    lp = C.lp_inputs(T, V, seed + 1)
    if flavour == "neginf":
        g = np.random.default_rng(seed + 2)
        hole = g.random((T, V)) < 0.15
        hole[:, 0] = False                       # never a whole row: the blank stays
        lp = np.where(hole, NEG, lp)
    return lp, lab, T


_REF = {}


def case_ref(case):
    """The case's inputs and float64 reference, computed once and shared (nobody writes into it)."""
    if case[0] not in _REF:
        lp, lab, T = case_inputs(case)
        _REF[case[0]] = (lp, lab, T, post_ref(lp, lab, T))
    return _REF[case[0]]
