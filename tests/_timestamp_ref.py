"""The timestamp grammar (include/tethys_mi.h, "Timestamp rules" a - g) restated in plain Python / numpy: rules a - f as a
predicate per column over integers, rule g in fp64, and one full constrained decode step.  Nothing here is shared with
the kernels; the bit-set helpers and the constrained logit z' are tests/_constrain_ref.py's.

Rule g compares lse_ts (the logsumexp of z' over the timestamp columns that are not banned) with max_below (the max of
z' over the below columns that are not banned).  The kernel's two sides carry the errors tests/_constrain_ref.py and
tests/_sample_ref.py already derive - nothing new:
  |max_below32 - max_below| <= bz',   bz' = constrained_bound(REL * scale)       (a max moves by at most its inputs' error)
  |lse_ts32 - lse_ts|       <= bl',   bl' = constrained_bound(REL * (scale + |lse_ts|))   (REL's own lse term: the fold)
so a row is DECIDED when |lse_ts - max_below| > bz' + bl', and a kernel must match every decided row.  On exact-score
inputs (``planted_case``) scale's term is 0: ``b_scale=0`` leaves the fold's REL * |lse_ts| and the penalty's rounding."""
import numpy as np

import _constrain_ref as C
import _sample_ref as S


def is_ts(x, tb, V):
    return tb <= x < V


def row_state(g, tb, V):
    """g: the generated tokens -> (n, last, pen, tl or None)."""
    n = len(g)
    last = n >= 1 and is_ts(g[n - 1], tb, V)
    pen = n < 2 or is_ts(g[n - 2], tb, V)
    stamps = [x for x in g if is_ts(x, tb, V)]
    return n, last, pen, (stamps[-1] if stamps else None)


def rule_bans(row, t, P, V, tb, no_ts, eos, max_initial, max_ts):
    """Rules a - f for one prefix row (columns [0, t) are read) -> bool [V]: the columns the rules ban."""
    g = [int(v) for v in row[1 + P:t]]
    n, last, pen, tl = row_state(g, tb, V)
    out = np.zeros(V, dtype=bool)
    for c in range(V):
        ts, below = c >= tb, c < tb
        ban = (no_ts >= 0 and c == no_ts) or (ts and c > tb + max_ts)                    # a
        if n == 0:
            ban |= below or (ts and max_initial >= 0 and c > tb + max_initial)          # b
        if last and pen:
            ban |= ts                                                                    # c
        if last and not pen:
            ban |= below and c != eos                                                    # d
        if tl is not None:
            ban |= ts and (c < tl if (last and not pen) else c <= tl)                    # e, f
        out[c] = ban
    return out


def rule_bans_fast(row, t, P, V, tb, no_ts, eos, max_initial, max_ts):
    """``rule_bans`` by slices (for V = 51865; tests/test_timestamp_cpu.py shows the two agree on tiny vocabularies)."""
    g = [int(v) for v in row[1 + P:t]]
    n, last, pen, tl = row_state(g, tb, V)
    out = np.zeros(V, dtype=bool)
    if 0 <= no_ts < V:
        out[no_ts] = True
    out[min(V, tb + max_ts + 1):] = True
    if n == 0:
        out[:tb] = True
        if max_initial >= 0:
            out[min(V, tb + max_initial + 1):] = True
    if last and pen:
        out[tb:] = True
    if last and not pen:
        keep = out[eos] if 0 <= eos < tb else None
        out[:tb] = True
        if keep is not None:
            out[eos] = keep
    if tl is not None:
        out[tb:(tl if (last and not pen) else tl + 1)] = True
    return out


def apply_rules(prefix, t, P, V, tb, no_ts, eos, max_initial, max_ts, banned, fast=None):
    """tmi_timestamp_rules: banned uint32 [M, >= W] -> a copy with the rules' bits OR-ed into the first W words."""
    fn = rule_bans_fast if (V > 4096 if fast is None else fast) else rule_bans
    out = np.array(banned, dtype=np.uint32, copy=True)
    W = C.words(V)
    for r in range(len(prefix)):
        out[r, :W] |= C.bitset(np.nonzero(fn(prefix[r], t, P, V, tb, no_ts, eos, max_initial, max_ts))[0], V)
    return out


def gate_ref(zp, tb, b_below=0.0, b_lse=0.0):
    """Rule g on z' [M, V] fp64 (-inf: banned) -> fired [M] bool, decided [M] bool, lse_ts [M], max_below [M]."""
    zp = np.asarray(zp, dtype=np.float64)
    M = zp.shape[0]
    lse = C.lse_rows(zp[:, tb:]) if zp.shape[1] > tb else np.full(M, -np.inf)
    below = zp[:, :tb].max(axis=1) if tb > 0 else np.full(M, -np.inf)
    with np.errstate(invalid="ignore"):
        fired = lse > below
        gap = np.abs(lse - below)
    both_inf = np.isinf(lse) & np.isinf(below)
    margin = np.broadcast_to(np.asarray(b_below, np.float64) + np.asarray(b_lse, np.float64), (M,))
    decided = both_inf | (np.isinf(lse) ^ np.isinf(below)) | (gap > margin)
    return fired & ~both_inf, decided, lse, below


def gate_bounds(zp, tb, scale, penalty):
    """(b_below, b_lse) of the module docstring, per row; ``scale`` = 0 on exact-score inputs."""
    lse = C.lse_rows(np.asarray(zp)[:, tb:])
    fin = np.where(np.isfinite(lse), np.abs(lse), 0.0)
    scale = np.broadcast_to(np.asarray(scale, np.float64), fin.shape)
    return C.constrained_bound(S.REL * scale, zp, penalty), C.constrained_bound(S.REL * (scale + fin), zp, penalty)


def gate_banned(banned, fired, tb, V):
    """The banned words after the gate: the below columns OR-ed in on the rows that fired."""
    out = np.array(banned, dtype=np.uint32, copy=True)
    below = C.bitset(range(tb), V)
    out[np.asarray(fired, bool), :C.words(V)] |= below
    return out


def step_ref(row, t, P, z, V, tb, no_ts, eos, max_initial, max_ts, seen=None, banned=None, penalty=1.0, b=0.0):
    """One full constrained decode step of one row: the caller's sets, rules a - f, z', rule g -> (banned bool [V] after
    everything, z' after everything, fired, decided)."""
    ban = C.to_bool(banned, V) if banned is not None else np.zeros(V, bool)
    ban = ban | (rule_bans_fast if V > 4096 else rule_bans)(row, t, P, V, tb, no_ts, eos, max_initial, max_ts)
    zp = C.constrain(np.asarray(z, np.float64)[None], None if seen is None else seen[None], C.bitset(np.nonzero(ban)[0], V)[None],
                     penalty)
    fired, decided, _, _ = gate_ref(zp, tb, b, b)
    if fired[0]:
        ban = ban.copy()
        ban[:tb] = True
        zp[0, :tb] = -np.inf
    return ban, zp[0], bool(fired[0]), bool(decided[0])


def grammar_ok(g, V, tb, no_ts, eos, max_initial, max_ts):
    """Whether every token of g (cut before the first EOS) was allowed by rules a - f given the tokens before it; -> the
    index of the first offender, or -1."""
    g = [int(v) for v in g]
    if eos in g:
        g = g[:g.index(eos) + 1]
    for i, x in enumerate(g):
        row = [0] + g[:i]
        if not 0 <= x < V or rule_bans_fast(row, 1 + i, 0, V, tb, no_ts, eos, max_initial, max_ts)[x]:
            return i
    return -1


# ----------------------------------------------------------------------------- inputs of tests/test_timestamp_kernels_gpu.py
RULE_MS, RULE_SHAPES, RULE_PS = (1, 5, 17), ((51865, 50364), (200, 137)), (0, 3)
SENTINEL = C.SENTINEL


def rule_case(M, V, tb, P):
    """One tmi_timestamp_rules input: rows cycling through the grammar's states - n = 0; an opening timestamp; text behind
    it; a closing timestamp (single); a closing/opening pair; text behind a pair; tl at tb + max_ts (closing, then pair);
    an id outside [0, V) as the last token; a row of text only; n = 2 with two timestamps.  Rows have different
    lengths n <= t - 1 - P only through their content: every row is read to t, so shorter states are padded IN FRONT with
    text.  The columns from t on hold timestamps that would change the state if read.  The incoming banned words hold
    random bits (and EOS banned on every third row), bits at or above V clear, and a sentinel word past W."""
    rng = np.random.RandomState(100 * M + V % 1000 + 7 * P)
    nts = V - tb
    max_ts = min(1500, nts - 1) - 2
    max_initial = 5
    eos, no_ts = 2, tb - 1
    a, b2 = tb + 3, tb + 9
    top = tb + max_ts
    states = [
        ("n0", []),
        ("open", [a]),
        ("text", [a, 7]),
        ("closing", [a, 7, b2]),
        ("pair", [a, 7, b2, b2]),
        ("text2", [a, 7, b2, b2, 9]),
        ("closing_top", [a, 7, top]),
        ("pair_top", [a, 7, top, top]),
        ("invalid_last", [a, 7, V]),
        ("invalid_neg", [a, -1]),
        ("text_only", [5, 6]),
        ("two_ts", [a, a + 1]),
        ("big_invalid", [a, 2 ** 31 - 1, b2]),
    ]
    nmax = max(len(s) for _, s in states)
    cases = []
    for fill in (0, 4):  # n exactly the state's, and the state behind 4 text tokens
        t = 1 + P + nmax + fill
        ld = t + 3
        prefix = np.full((M, ld), 11, dtype=np.int64)
        names = []
        for r in range(M):
            name, st = states[(r + M) % len(states)]
            names.append(name)
            row = [50] + list(rng.randint(20, 40, size=P)) + [11] * (t - 1 - P - len(st)) + st
            prefix[r, :t] = row
            prefix[r, t:] = tb + 1
        W = C.words(V)
        banned = np.zeros((M, W + 1), np.uint32)
        for r in range(M):
            ids = set(int(v) for v in rng.randint(0, V, size=9))
            if r % 3 == 0:
                ids.add(eos)
            banned[r, :W] = C.bitset(sorted(ids), V)
        banned[:, W] = SENTINEL
        cases.append(dict(M=M, V=V, tb=tb, P=P, t=t, ld=ld, prefix=prefix.astype(np.int32), banned=banned, names=names,
                          eos=eos, no_ts=no_ts, max_initial=max_initial, max_ts=max_ts, W=W))
    # n == 0 and n == 1 for every row (t = 1 + P and 2 + P): the states that need a short prefix
    for n in (0, 1):
        t = 1 + P + n
        prefix = np.full((M, t + 2), tb + 1, dtype=np.int64)
        prefix[:, 0] = 50
        prefix[:, 1:1 + P] = 21
        if n:
            prefix[:, 1 + P] = [tb + (r % 3) if r % 2 == 0 else 8 for r in range(M)]
        W = C.words(V)
        banned = np.zeros((M, W + 1), np.uint32)
        banned[:, W] = SENTINEL
        cases.append(dict(M=M, V=V, tb=tb, P=P, t=t, ld=t + 2, prefix=prefix.astype(np.int32), banned=banned,
                          names=[f"n{n}"] * M, eos=eos, no_ts=no_ts, max_initial=max_initial, max_ts=max_ts, W=W))
    return cases


def rule_expected(c):
    return apply_rules(c["prefix"], c["t"], c["P"], c["V"], c["tb"], c["no_ts"], c["eos"], c["max_initial"], c["max_ts"],
                       c["banned"])


GATE_D, GATE_MS, GATE_SMALL, GATE_LARGE = 64, (1, 8, 16, 17), (200, 137), (51865, 50364)
GATE_PENALTY = 2.0
PATTERNS = ("fire_single", "no_fire", "spread", "ts_banned", "below_banned", "penalty_fires", "all_banned", "random_sets")
_PLANTED = {}


def planted_case(M, V, tb):
    """Exact-score inputs of tmi_lm_head_timestamp_gate (tests/_constrain_ref.head_case's recipe: x in {-1, 0, 1}, w
    multiples of 1/8, every partial sum exact in fp32 and bf16 in any order; penalty 2 keeps z' exact).  The first 16
    features are a one-hot of the row's pattern, so rows 0 .. 15 of w are per-pattern offsets on every column's logit;
    the patterns, (r + M) % 8:
      fire_single    one timestamp column at base + 12: fires.
      no_fire        one text column at base + 12: does not fire.
      spread         no base; every timestamp column at 1, the best text column at 3, the rest 0: no single timestamp
                     column beats the text column, lse_ts = 1 + log(V - tb) > 3 does: the LSE, not a max, fires it.
      ts_banned      the timestamp columns + 12 and every one of them banned: lse_ts = -inf, does not fire.
      below_banned   a text column + 12 and every below column banned: max_below = -inf, fires (and adds no new bit).
      penalty_fires  no base; the best text column at 8 and SEEN (z' = 4 under penalty 2), one timestamp column at 6,
                     the other timestamps at -8: fires only because of the penalty.
      all_banned     every column banned: -inf on both sides, does not fire.
      random_sets    30 % seen, 20 % banned over the base logits.
    Bits at or above V of the last word are set in both sets (a caller's garbage) and a sentinel word follows."""
    key = (M, V, tb)
    if key in _PLANTED:
        return _PLANTED[key]
    d = GATE_D
    rng = np.random.RandomState(31 * M + V % 1000)
    VP = (V + 7) // 8 * 8
    x = np.zeros((M, d), np.float32)
    w = np.zeros((d, VP), np.float32)
    w[16:, :V] = rng.randint(-4, 5, size=(d - 16, V)) / 8.0
    W = C.words(V)
    seen, banned = np.zeros((M, W + 1), np.uint32), np.zeros((M, W + 1), np.uint32)
    text_col, ts_col = 3 % tb, tb + (5 % (V - tb))
    w[0, ts_col] = 12.0
    w[1, text_col] = 12.0
    w[2, tb:V], w[2, text_col] = 1.0, 3.0
    w[3, tb:V] = 12.0
    w[4, text_col] = 12.0
    w[5, tb:V], w[5, ts_col], w[5, text_col] = -8.0, 6.0, 8.0
    names = []
    for r in range(M):
        p = (r + M) % 8
        names.append(PATTERNS[p])
        x[r, p] = 1.0
        if PATTERNS[p] not in ("spread", "penalty_fires"):
            x[r, 16:] = rng.randint(-1, 2, size=d - 16)
        s_ids, b_ids = [], []
        if PATTERNS[p] == "ts_banned":
            b_ids = list(range(tb, V))
        elif PATTERNS[p] == "below_banned":
            b_ids = list(range(tb))
        elif PATTERNS[p] == "penalty_fires":
            s_ids = [text_col]
        elif PATTERNS[p] == "all_banned":
            b_ids = list(range(V))
        elif PATTERNS[p] == "random_sets":
            s_ids, b_ids = list(np.nonzero(rng.rand(V) < 0.3)[0]), list(np.nonzero(rng.rand(V) < 0.2)[0])
        seen[r, :W], banned[r, :W] = C.bitset(s_ids, V), C.bitset(b_ids, V)
        if V & 31:
            hi = np.uint32((0xFFFFFFFF << (V & 31)) & 0xFFFFFFFF)
            seen[r, W - 1] |= hi
            banned[r, W - 1] |= hi
    seen[:, W], banned[:, W] = SENTINEL, SENTINEL
    z = x.astype(np.float64) @ w[:, :V].astype(np.float64)
    zp = C.constrain(z, seen, banned, GATE_PENALTY)
    bb, bl = gate_bounds(zp, tb, 0.0, GATE_PENALTY)
    fired, decided, lse, below = gate_ref(zp, tb, bb, bl)
    _PLANTED[key] = dict(x=x, w=w, z=z, zp=zp, seen=seen, banned=banned, VP=VP, W=W, names=names, fired=fired, decided=decided,
                         lse=lse, below=below)
    return _PLANTED[key]


RANDOM_CASES = (("bf16", 64, 200, 137, 40, 21), ("fp32", 64, 200, 137, 40, 22))  # (dtype, d, V, tb, M, seed)
RANDOM_PENALTY, RANDOM_CAP = 1.3, 0.05
_RANDOM = {}


def random_case(wdt, d, V, tb, M, seed):
    """Random inputs with LayerNorm (tests/_constrain_ref.random_case's recipe; the M decoded rows are every third row of
    x) and random sets; row r has a further r / M of its timestamp columns banned, so that both outcomes of the rule
    occur."""
    import torch
    key = (wdt, d, V, tb, M, seed)
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
    W = C.words(V)
    sb, bb = rng.rand(M, V) < 0.3, rng.rand(M, V) < 0.2
    for r in range(M):  # row r keeps about (M - r) / M of its timestamp columns: lse_ts falls from row to row
        bb[r, tb:] |= rng.rand(V - tb) < r / M
    seen = np.stack([C.bitset(np.nonzero(sb[r])[0], V) for r in range(M)])
    banned = np.stack([C.bitset(np.nonzero(bb[r])[0], V) for r in range(M)])
    zp = C.constrain(z, seen, banned, RANDOM_PENALTY)
    b_below, b_lse = gate_bounds(zp, tb, scale, RANDOM_PENALTY)
    fired, decided, lse, below = gate_ref(zp, tb, b_below, b_lse)
    _RANDOM[key] = dict(w=w, gamma=gamma, beta=beta, x=x, seen=seen, banned=banned, z=z, zp=zp, scale=scale, VP=VP, W=W,
                        fired=fired, decided=decided, lse=lse, below=below)
    return _RANDOM[key]
