"""Decode constraints (include/tethys_mi.h, "Decode constraints") restated in plain Python / numpy, fp64: the set builder
of tmi_decode_constraints, the constrained logit z', and the three choice rules on z' - the rank / choose / decided-row
machinery is tests/_sample_ref.py's, fed z' instead of z.  Nothing here is shared with the kernels.

Every row reports whether it is DECIDED under a bound ``b`` on the kernel's scores (b = 0 on exact-score inputs).  On
rounded inputs the bound of the unconstrained score s = z / T, ``b`` (tests/_sample_ref.py: REL * (scale + |lse|)), grows
by the penalty's own operation.  The kernel holds z32 with |z32 - z| <= bz and computes z'32 = fl(z32 / p) or fl(z32 * p):
  |z32 op p - z op p| <= bz * max(p, 1 / p)       (also when z32 and z differ in sign: then |z32| + |z| <= bz, and the
                                                    two branches differ by at most |z32| / p + |z| p)
  |fl(y) - y|         <= 2^-24 |y|                 (one correctly rounded fp32 operation: half an ulp)
so on the s scale  b' = b * max(p, 1 / p) + 2^-24 * max_n |z'[n]| / T   (``constrained_bound``).

``MUTATIONS`` lists wrong readings of the rule; ``mutation=`` makes the reference compute that reading instead.
tests/test_constrain_cpu.py checks that each of them changes the expected result of at least one input of the GPU
kernel tests - all but ``penalty_divides_at_zero``, which cannot change anything: 0 / p and 0 * p are the same fp32 zero
for every finite p > 0, so "z >= 0" and "z > 0" are one rule (the test asserts exactly that)."""
import numpy as np

import _sample_ref as S

MUTATIONS = (
    "penalty_always_multiplies",      # z * p also where z > 0
    "penalty_divides_at_zero",        # z >= 0 divides (equivalent: see above)
    "seen_without_start",             # the seen set skips column 0
    "ngram_window_starts_late",       # a match at column 0 is missed
    "ngram_window_ends_early",        # the match whose token is the prefix's last is missed
    "ngram_overlap_dropped",          # a match whose context overlaps the suffix is dropped
    "begin_suppress_every_step",      # begin_suppress_tokens banned at every step
    "static_dropped_without_ngram",   # the static bans are lost when the n-gram size is 0
    "high_bits_left_set",             # bits at or above V of the last word are not cleared
)
EQUIVALENT = ("penalty_divides_at_zero",)
INVALID_IDS = (-1, None, 2 ** 31 - 1)  # (None: V)


def words(V):
    return (int(V) + 31) // 32


def bitset(ids, V, W=None):
    out = np.zeros(words(V) if W is None else W, dtype=np.uint32)
    ids = np.asarray(list(ids), dtype=np.int64)
    if len(ids):
        np.bitwise_or.at(out, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return out


def to_bool(bits, V):
    """uint32 [..., >= W] -> bool [..., V]: bit n & 31 of word n >> 5 (bits at or above V are not looked at)."""
    n = np.arange(V)
    return ((np.asarray(bits, dtype=np.uint32)[..., n >> 5] >> (n & 31).astype(np.uint32)) & 1).astype(bool)


def static_ids(suppress, begin, first, mutation=None):
    """The ids banned at every position of a step: suppress, and begin_suppress at the first generated step."""
    if first or mutation == "begin_suppress_every_step":
        return sorted(set(suppress) | set(begin))
    return sorted(set(suppress))


def build_sets(prefix, t, V, static_words=None, ngram=0, mutation=None):
    """tmi_decode_constraints: prefix [M, ld] (columns [0, t) are read) -> seen, banned uint32 [M, W]."""
    M, W = len(prefix), words(V)
    seen, banned = np.zeros((M, W), np.uint32), np.zeros((M, W), np.uint32)

    def put(dst, x):
        if 0 <= x < V:
            dst[x >> 5] |= np.uint32(1 << (x & 31))

    for r in range(M):
        row = [int(v) for v in prefix[r][:t]]
        for x in row[1 if mutation == "seen_without_start" else 0:]:
            put(seen[r], x)
        if static_words is not None and not (mutation == "static_dropped_without_ngram" and ngram == 0):
            banned[r] |= np.asarray(static_words, dtype=np.uint32)[:W]
        g = ngram - 1
        if ngram >= 1 and t >= g:
            suffix = row[t - g:t]
            first_j = 1 if mutation == "ngram_window_starts_late" else 0
            last_j = t - 1 - g - (1 if mutation == "ngram_window_ends_early" else 0)
            for j in range(first_j, last_j + 1):
                if mutation == "ngram_overlap_dropped" and g > 0 and j + g - 1 >= t - g:
                    continue
                if row[j:j + g] == suffix:
                    put(banned[r], row[j + g])
        if V & 31 and mutation != "high_bits_left_set":
            mask = np.uint32((1 << (V & 31)) - 1)
            seen[r, W - 1] &= mask
            banned[r, W - 1] &= mask
    return seen, banned


def constrain(z, seen, banned, penalty, mutation=None):
    """z [M, V] fp64 -> z': -inf where banned, z / p (z > 0) or z * p (z <= 0) where seen."""
    z = np.asarray(z, dtype=np.float64)
    V = z.shape[1]
    sb = to_bool(seen, V) if seen is not None else np.zeros(z.shape, bool)
    bb = to_bool(banned, V) if banned is not None else np.zeros(z.shape, bool)
    if mutation == "penalty_always_multiplies":
        pen = z * penalty
    elif mutation == "penalty_divides_at_zero":
        pen = np.where(z >= 0, z / penalty, z * penalty)
    else:
        pen = np.where(z > 0, z / penalty, z * penalty)
    zp = np.where(sb, pen, z)
    zp[bb] = -np.inf
    return zp


def constrained_bound(b, zp, penalty, T=1.0):
    """b' of the module docstring, per row."""
    big = np.where(np.isfinite(zp), np.abs(zp), 0.0).max(axis=1)
    return np.asarray(b, dtype=np.float64) * max(penalty, 1.0 / penalty) + 2.0 ** -24 * big / T


def _gaps_clear(vals, b):
    """vals [n] sorted desc (may hold -inf): every neighbouring pair further apart than 2b (b = 0, or two -inf: the
    column order decides, and that is exact)."""
    ok = True
    for a, c in zip(vals[:-1], vals[1:]):
        if b == 0.0 or (np.isinf(a) and np.isinf(c)):
            continue
        ok &= bool(a - c > 2 * b)
    return ok


def lse_rows(sp):
    """logsumexp over the columns that are not -inf; -inf for a row without one."""
    out = np.full(sp.shape[0], -np.inf)
    for r in range(sp.shape[0]):
        fin = sp[r][np.isfinite(sp[r])]
        if len(fin):
            out[r] = fin.max() + np.log(np.exp(fin - fin.max()).sum())
    return out


def argmax_ref(zp, b=0.0):
    """-> token [M] (ties: the smaller column; every column banned: column 0), decided [M]."""
    order = np.argsort(-zp, axis=1, kind="stable")[:, :2]
    bb = np.broadcast_to(np.asarray(b, dtype=np.float64), (zp.shape[0],))
    dec = np.array([_gaps_clear(zp[r, order[r]], float(bb[r])) for r in range(zp.shape[0])])
    return order[:, 0], dec


def topk_ref(sp, N, b=0.0):
    """-> ids [M, N], logprobs [M, N] (-inf for a banned column), lse [M], decided [M]."""
    M = sp.shape[0]
    order = np.argsort(-sp, axis=1, kind="stable")[:, :N + 1]
    lse = lse_rows(sp)
    vals = np.take_along_axis(sp, order, axis=1)
    with np.errstate(invalid="ignore"):
        lp = np.where(np.isinf(vals), -np.inf, vals - lse[:, None])
    bb = np.broadcast_to(np.asarray(b, dtype=np.float64), (M,))
    dec = np.array([_gaps_clear(vals[r], float(bb[r])) for r in range(M)])
    return order[:, :N], lp[:, :N], lse, dec


def sample_ref(sp, seed, top_k, top_p, finished=None, suppress_id=-1, pad_id=0, b=0.0):
    """s' [M, V] (banned: -inf) -> token [M], logprob [M], decided [M], allowed (list of column arrays per row).  A
    finished row and a row without a column to draw write pad_id and log-probability 0."""
    sp = np.array(sp, dtype=np.float64)
    M = sp.shape[0]
    if suppress_id >= 0:
        sp[:, suppress_id] = -np.inf
    fin = np.zeros(M, bool) if finished is None else np.asarray(finished).astype(bool)
    live = np.nonzero(~fin & np.isfinite(sp).any(axis=1))[0]
    tok, lp, dec = np.full(M, pad_id, np.int64), np.zeros(M), np.ones(M, bool)
    allowed = [np.array([pad_id])] * M
    if len(live):
        s, lse, top = S.rank(sp[live])
        bb = np.broadcast_to(np.asarray(b, dtype=np.float64), (M,))[live]
        if top_k:
            t2, l2, d2, a2 = S.choose_topk(s, lse, top, seed, top_k, top_p, b=bb, rows=live)
        else:
            t2, l2, d2, second = S.choose_gumbel(s, lse, seed, b=bb, rows=live)
            a2 = np.stack([t2, second], 1)
        for i, r in enumerate(live):
            tok[r], lp[r], dec[r], allowed[r] = t2[i], l2[i], d2[i], a2[i]
    return tok, lp, dec, allowed


# ----------------------------------------------------------------------------- inputs of tests/test_constrain_kernels_gpu.py
# Built on the host, so that tests/test_constrain_cpu.py can show from the reference alone that every mutation changes the
# expected result of one of them, and that the undecided rows stay under the cap for the very seeds the GPU tests use.
SET_MS, SET_VS, SET_NGRAMS = (1, 5, 17), (33, 128, 160, 51865), (0, 1, 2, 3, 5)
SENTINEL = 0x5A5A5A5A


def set_ts(ngram):
    return sorted({t for t in (1, 2, ngram - 1, ngram, 40, 448) if t >= 1})


def set_case(M, V, t, ngram):
    """One tmi_decode_constraints input.  Rows by r % 4: 0 the suffix repeated at column 0; 1 a copy of the suffix whose
    following token sits right before the suffix; 2 a run of one token; 3 a last token that occurs nowhere else (no
    match for ngram >= 2).  The filler comes from a small alphabet, so matches happen on their own too.  Column 0 holds
    V - 2, found nowhere else in rows 1 and 3 (mod 4); odd rows with t >= 6 get the ids -1, V and 2^31 - 1 somewhere;
    the 6 columns from t on hold V - 1 (and the row's suffix again), which would change both sets if read."""
    rng = np.random.RandomState(1000 * M + 10 * t + ngram + V % 997)
    g = max(ngram - 1, 0)
    ld = t + 6
    alpha = max(2, min(V - 3, 6))
    prefix = rng.randint(0, alpha, size=(M, ld)).astype(np.int64)
    for r in range(M):
        row = prefix[r]
        if r % 4 == 2:
            row[:t] = r % alpha
        else:
            row[0] = V - 2
            if r % 4 == 0 and 0 < g < t:  # (period t - g: row[t - g + k] == row[k] for every k < g)
                for i in range(t - g, t):
                    row[i] = row[i - (t - g)]
            if r % 4 == 1 and g > 0 and t - 2 * g - 1 >= 0:
                row[t - 2 * g - 1:t - g - 1] = row[t - g:t]
            if r % 4 == 3:
                row[t - 1] = V - 3
        if r % 2 == 1 and t >= 6:
            for x, pos in zip(INVALID_IDS, rng.choice(np.arange(1, t), size=3, replace=False)):
                row[pos] = V if x is None else x
        row[t:] = V - 1
        if g and t >= g:
            tail = row[t - g:t][:min(g, 5)]
            row[t + 1:t + 1 + min(g, 5)] = np.where((tail >= 0) & (tail < V), tail, V - 1)
    first = (M + t + ngram) % 2 == 0
    suppress = sorted({1 % V, (V // 2) % V, V - 1})
    begin = sorted({2 % V, (V // 3) % V})
    has_static = (M + t) % 3 != 0
    W = words(V)
    return {"M": M, "V": V, "t": t, "ngram": ngram, "ld": ld, "prefix": prefix.astype(np.int32), "first": first,
            "suppress": suppress, "begin": begin, "has_static": has_static, "bits_ld": W + (2 if (M + ngram) % 2 else 0)}


def set_case_static(c, mutation=None):
    """The static_banned words the caller passes in (None: NULL).  Bits at or above V of the last word are SET here - a
    caller's garbage - and the kernel has to clear them."""
    if not c["has_static"]:
        return None
    w = bitset(static_ids(c["suppress"], c["begin"], c["first"], mutation), c["V"])
    if c["V"] & 31:
        w[-1] |= np.uint32((0xFFFFFFFF << (c["V"] & 31)) & 0xFFFFFFFF)
    return w


def set_case_expected(c, mutation=None):
    return build_sets(c["prefix"], c["t"], c["V"], set_case_static(c, mutation), c["ngram"], mutation)


def set_cases(V=None):
    for v in SET_VS if V is None else (V,):
        for M in SET_MS:
            for ngram in SET_NGRAMS:
                for t in set_ts(ngram):
                    yield set_case(M, v, t, ngram)


HEAD_DS, HEAD_VS, HEAD_MS, HEAD_PENALTIES = (64, 384), (130, 1000), (1, 3, 16, 17, 40), (2.0, 0.5)
HEAD_SUPPRESS, HEAD_ZERO_COL, HEAD_PAD = 9, 5, 3
HEAD_TOPK_N = 6
HEAD_SAMPLE = ((8, 1.0, 1.0), (50, 0.9, 2.0), (1, 1.0, 0.5), (0, 1.0, 1.0))  # (top_k, top_p, temperature)
CAP = 0.05
_HEAD = {}


def head_case(d, V, M):
    """Exact-score inputs of the _c LM heads: x in {-1, 0, 1} [M, d], w multiples of 1/8 in [-1/2, 1/2] [d, VP] (column
    HEAD_ZERO_COL and the pad columns zero), so every partial sum is a multiple of 1/8 below 2^8 - exact in fp32 and bf16
    in any order - and penalties 2 and 1/2 and temperatures 1/2, 1, 2 keep z' and s exact too.  The sets, by row pattern
    (r + d + V) % 8: 0 the winner banned, and every column of its workgroup's 128 that beats the best one outside (the
    new winner lives in another workgroup); 1 the winner seen (z > 0); 2 every column with z >= 0 banned and the winner of
    the rest (z < 0) seen; 3 every z > 0 banned and the first z == 0 column seen; 4 the winner seen and banned; 5 all but
    one column banned; 6 every column banned; 7 random sets.  Every row has the bits of the pad positions (columns >= V
    of the last word) set in both sets.  -> dict(x, w, z, scale, seen, banned uint32 [M, W + 1], finished, VP)."""
    key = (d, V, M)
    if key in _HEAD:
        return _HEAD[key]
    rng = np.random.RandomState(7 * d + V + 100 * M)
    VP = (V + 7) // 8 * 8
    x = rng.randint(-1, 2, size=(M, d)).astype(np.float32)
    w = np.zeros((d, VP), dtype=np.float32)
    w[:, :V] = rng.randint(-4, 5, size=(d, V)) / 8.0
    w[:, HEAD_ZERO_COL] = 0.0
    z = x.astype(np.float64) @ w[:, :V].astype(np.float64)
    scale = (np.abs(x.astype(np.float64)) @ np.abs(w[:, :V].astype(np.float64))).max(1) + 1.0
    W = words(V)
    seen, banned = np.zeros((M, W + 1), np.uint32), np.zeros((M, W + 1), np.uint32)
    patterns = []
    for r in range(M):
        pat = (r + d + V) % 8
        zr = z[r]
        order = np.argsort(-zr, kind="stable")
        s_ids, b_ids = [], []
        if pat == 0:
            blk = order[0] // 128
            outside = [c for c in order if c // 128 != blk]
            b_ids = [c for c in order if c // 128 == blk and (zr[c], -c) >= (zr[outside[0]], -outside[0])]
        elif pat == 1:
            s_ids = [order[0]]
        elif pat == 2:
            b_ids = list(np.nonzero(zr >= 0)[0])
            rest = [c for c in order if zr[c] < 0]
            s_ids = rest[:1]
        elif pat == 3:
            b_ids = list(np.nonzero(zr > 0)[0])
            s_ids = [int(np.nonzero(zr == 0)[0][0])]
        elif pat == 4:
            s_ids, b_ids = [order[0]], [order[0]]
        elif pat == 5:
            b_ids = [c for c in range(V) if c != (7 * r + 3) % V]
        elif pat == 6:
            b_ids = list(range(V))
        else:
            s_ids = list(np.nonzero(rng.rand(V) < 0.3)[0])
            b_ids = list(np.nonzero(rng.rand(V) < 0.2)[0])
        seen[r, :W], banned[r, :W] = bitset(s_ids, V), bitset(b_ids, V)
        if V & 31:
            hi = np.uint32((0xFFFFFFFF << (V & 31)) & 0xFFFFFFFF)
            seen[r, W - 1] |= hi
            banned[r, W - 1] |= hi
        patterns.append(pat)
    seen[:, W], banned[:, W] = SENTINEL, SENTINEL
    finished = (np.arange(M) % 5 == 2).astype(np.int32)
    _HEAD[key] = dict(x=x, w=w, z=z, scale=scale, seen=seen, banned=banned, finished=finished, VP=VP, patterns=patterns)
    return _HEAD[key]


def head_seed(d, V, M, penalty, top_k):
    return 13 * d + V + 1000 * M + int(penalty * 4) + 31 * top_k


def head_expected(d, V, M, penalty, mutation=None):
    """Everything the exact-score GPU test compares, at b = 0: {"argmax": (tok, dec), "topk": (ids, lp, lse, dec) at
    T = 1, "sample": {(top_k, top_p, T): (tok, lp, dec, allowed)}}."""
    c = head_case(d, V, M)
    zp = constrain(c["z"], c["seen"], c["banned"], penalty, mutation)
    out = {"zp": zp, "argmax": argmax_ref(zp), "topk": topk_ref(zp, HEAD_TOPK_N), "sample": {}}
    for top_k, top_p, T in HEAD_SAMPLE:
        out["sample"][(top_k, top_p, T)] = sample_ref(zp / T, head_seed(d, V, M, penalty, top_k), top_k, top_p,
                                                      finished=c["finished"], suppress_id=HEAD_SUPPRESS, pad_id=HEAD_PAD)
    return out


RANDOM_T, RANDOM_PENALTY, RANDOM_N = 0.7, 1.3, 6
RANDOM_CASES = (("bf16", 384, 1000, 40, 11), ("fp32", 384, 1000, 40, 12), ("bf16", 768, 51865, 16, 13))  # (.., input seed)
RANDOM_SAMPLE = ((8, 1.0), (50, 0.9), (0, 1.0))
_RANDOM = {}


def random_case(wdt, d, V, M, seed):
    """Random inputs with LayerNorm (tests/_sample_ref.random_inputs' recipe; the M decoded rows are every third row of
    x), random sets (30 % seen, 20 % banned, and the fp64 winner of every other row seen, of every fourth banned) ->
    torch CPU tensors w, gamma, beta, x [3 M, d], and numpy seen, banned, z [M, V] (fp64, LayerNorm applied), b [M] (the
    unconstrained bound at temperature RANDOM_T, without the |lse| term) and VP."""
    import torch
    key = (wdt, d, V, M, seed)
    if key in _RANDOM:
        return _RANDOM[key]
    g = torch.Generator().manual_seed(seed)
    VP = (V + 7) // 8 * 8
    w = torch.zeros(d, VP)
    w[:, :V] = torch.randn(d, V, generator=g) * d ** -0.5
    dt = torch.bfloat16 if wdt == "bf16" else torch.float32
    w = w.to(dt)
    gamma = 1 + 0.1 * torch.randn(d, generator=g)
    beta = 0.1 * torch.randn(d, generator=g)
    x = (torch.randn(M * 3, d, generator=g) * 2 + 0.5).to(dt)
    y = x[2::3].double()
    mu = y.mean(1, keepdim=True)
    var = ((y - mu) ** 2).mean(1, keepdim=True)
    y = (y - mu) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double()
    wd = w[:, :V].double()
    z = (y @ wd).numpy()
    scale = (y.abs() @ wd.abs()).max(1).values.numpy()
    rng = np.random.RandomState(seed)
    W = words(V)
    sb, bb = rng.rand(M, V) < 0.3, rng.rand(M, V) < 0.2
    win = z.argmax(1)
    for r in range(M):
        sb[r, win[r]] = r % 2 == 0 or sb[r, win[r]]
        bb[r, win[r]] = r % 4 == 1
    seen = np.stack([bitset(np.nonzero(sb[r])[0], V) for r in range(M)])
    banned = np.stack([bitset(np.nonzero(bb[r])[0], V) for r in range(M)])
    _RANDOM[key] = dict(w=w, gamma=gamma, beta=beta, x=x, seen=seen, banned=banned, z=z, scale=scale, VP=VP, W=W)
    return _RANDOM[key]


def random_expected(case):
    """The fp64 reference of one RANDOM_CASES entry with the derived bounds: zp, and per head the choice with its
    decided rows; ``b`` = b' of the module docstring on the head's own score scale."""
    wdt, d, V, M, seed = case
    c = random_case(*case)
    zp = constrain(c["z"], c["seen"], c["banned"], RANDOM_PENALTY)
    out = {"zp": zp}
    b_arg = constrained_bound(S.REL * c["scale"], zp, RANDOM_PENALTY)
    out["argmax"] = argmax_ref(zp, b_arg) + (b_arg,)
    sp = zp / RANDOM_T
    lse = lse_rows(sp)
    b_s = constrained_bound(S.REL * (c["scale"] / RANDOM_T + np.abs(lse)), zp, RANDOM_PENALTY, RANDOM_T)
    out["sp"], out["lse"], out["b"] = sp, lse, b_s
    out["topk"] = topk_ref(sp, RANDOM_N, b_s)
    out["sample"] = {(k, p): sample_ref(sp, 77 * d + M + 31 * k, k, p, b=b_s) for k, p in RANDOM_SAMPLE}
    return out


def cap_ok(decided, cap=CAP):
    return int((~np.asarray(decided)).sum()) <= cap * len(decided)


# ----------------------------------------------------------------------------- generate: the loop the oracle follows
def has_repeated_ngram(tokens, n):
    """Whether some n-gram occurs twice in the token list."""
    grams = [tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1)]
    return len(set(grams)) != len(grams)


def step_banned(prefix_row, V, ngram, suppress=(), begin=(), first=False):
    """The banned columns (bool [V]) of one row at one generate step."""
    static = bitset(static_ids(suppress, begin, first), V)
    _, banned = build_sets([list(prefix_row)], len(prefix_row), V, static, ngram)
    return to_bool(banned[0], V)
