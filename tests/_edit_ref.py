"""Reference for tmi_edit_distance (include/tethys_mi.h, "Error-rate evaluation"): a plain Python restatement of the
normalisation and of the rule, and two generators of cases.  No GPU, no torch."""
import numpy as np

STOP, SKIP = 50, (100, 110)  # ids the generators use for the stop token and the skip range; the alphabet stays below them


def normalise(row, length=None, cols=None, stop_id=-1, skip_lo=0, skip_hi=0):
    """The kept tokens of one row: its first min(len, cols) tokens (a negative len counts as 0), cut before the first
    stop_id (-1: no cut), without the tokens in [skip_lo, skip_hi)."""
    row = [int(x) for x in row]
    cols = len(row) if cols is None else int(cols)
    length = cols if length is None else int(length)
    row = row[:max(0, min(length, cols))]
    if stop_id != -1 and stop_id in row:
        row = row[:row.index(stop_id)]
    return [x for x in row if not (skip_lo <= x < skip_hi)]


def rule(h, r):
    """(d, sub, del, ins, n, m) of the header's table: candidates in the order diagonal, up, left; a later one replaces an
    earlier one only when its d is strictly smaller."""
    n, m = len(h), len(r)
    prev = [(j, 0, j, 0) for j in range(m + 1)]
    for i in range(1, n + 1):
        cur = [(i, 0, 0, i)]
        hi = h[i - 1]
        for j in range(1, m + 1):
            d, s, de, ins = prev[j - 1]
            if hi != r[j - 1]:
                d, s = d + 1, s + 1
            best = (d, s, de, ins)
            u = prev[j]
            if u[0] + 1 < best[0]:
                best = (u[0] + 1, u[1], u[2], u[3] + 1)
            l = cur[j - 1]
            if l[0] + 1 < best[0]:
                best = (l[0] + 1, l[1], l[2] + 1, l[3])
            cur.append(best)
        prev = cur
    return prev[m] + (n, m)


def reference(hyp, ref, hyp_len=None, ref_len=None, R=1, stop_id=-1, skip=(0, 0), hyp_cols=None, ref_cols=None):
    """What the kernel writes: int32 [N, 6], pair i = hypothesis i against reference i // R."""
    hyp, ref = np.asarray(hyp), np.asarray(ref)
    out = np.zeros((hyp.shape[0], 6), np.int32)
    refs = [normalise(ref[b], None if ref_len is None else ref_len[b], ref.shape[1] if ref_cols is None else ref_cols,
                      stop_id, skip[0], skip[1]) for b in range(ref.shape[0])]
    for i in range(hyp.shape[0]):
        h = normalise(hyp[i], None if hyp_len is None else hyp_len[i], hyp.shape[1] if hyp_cols is None else hyp_cols,
                      stop_id, skip[0], skip[1])
        out[i] = rule(h, refs[i // R])
    return out


def counts(out, R=1, valid=None):
    """The sums ``ops.edit_counts`` reports, from a [N, 6] table."""
    o = np.asarray(out, np.int64).reshape(-1, R, 6)
    first = o[:, 0]
    d = o[:, :, 0].copy()
    if valid is not None:
        v = np.asarray(valid, bool).copy()
        v[:, 0] = True
        d[~v] = 1 << 40
    c = {"n_edits": float(first[:, 0].sum()), "n_sub": float(first[:, 1].sum()), "n_del": float(first[:, 2].sum()),
         "n_ins": float(first[:, 3].sum()), "n_hyp_tokens": float(first[:, 4].sum()), "n_ref_tokens": float(first[:, 5].sum()),
         "n_exact": float((first[:, 0] == 0).sum()), "n_items": float(o.shape[0]), "n_oracle_edits": float(d.min(1).sum())}
    c["token_error_rate"] = c["n_edits"] / c["n_ref_tokens"] if c["n_ref_tokens"] else float("nan")
    c["oracle_error_rate"] = c["n_oracle_edits"] / c["n_ref_tokens"] if c["n_ref_tokens"] else float("nan")
    return c


def random_rows(rng, lengths, cols, alphabet=4, garbage=True, ld=None):
    """int32 [len(lengths), ld] rows: row i holds lengths[i] symbols of a small alphabet (so ties are everywhere), then
    garbage (-1 and 2^31 - 1 alternating) up to ld >= cols."""
    ld = cols if ld is None else ld
    rows = np.empty((len(lengths), ld), np.int32)
    rows[:, 0::2], rows[:, 1::2] = (-1, 2 ** 31 - 1) if garbage else (0, 0)
    for i, n in enumerate(lengths):
        rows[i, :n] = rng.integers(0, alphabet, n)
    return rows


def sprinkle(rng, row, n, p_skip=0.2, stop_at=None):
    """A raw row that normalises to row[:n] kept symbols mixed with skip-range tokens (and, with ``stop_at`` = the number of
    kept symbols before it, a stop token followed by more symbols that must not count)."""
    out = []
    for k in range(n):
        while rng.random() < p_skip:
            out.append(int(rng.integers(*SKIP)))
        if stop_at is not None and k == stop_at:
            out.append(STOP)
        out.append(int(row[k]))
    return out


def planted_case(m, sites, seed=0, first=False, last=False):
    """A pair with known operation counts.  The reference is m all-distinct ids.  ``sites`` is an ordered list of
    (kind, run): "s" replaces ``run`` consecutive reference tokens by fresh ids, "d" drops ``run`` consecutive reference
    tokens, "i" inserts ``run`` fresh ids.  Consecutive sites are separated by at least g = max(2, 1 + the second largest
    run among the "d" and "i" sites) reference tokens that the hypothesis keeps - two where every edit is a single token;
    ``first`` / ``last`` put the first / last site at the very start / end (otherwise at least g kept tokens precede /
    follow).  -> (hyp, ref, (k_s, k_d, k_i)) with k_* the total run lengths per kind.

    Why the rule must give exactly (k_s, k_d, k_i).  Every id occurs at most once on each side, so a diagonal step can be
    free only between a kept token and its own copy, and the copies are in the same order on both sides.  The alignment
    that matches every kept token with its copy pays one substitution per token of an "s" run, one deletion per token of
    a "d" run and one insertion per token of an "i" run: d <= k_s + k_d + k_i.  Any other alignment gives up the match of
    at least one kept token.  Giving up matches can only pay by pairing t deletions of one site with t insertions of
    ANOTHER site as substitutions (within a site there is only one kind, and a substitution cannot be made cheaper):
    that shifts the alignment by t across all the kept tokens between the two sites, at least g of them, each of which
    becomes a substitution - t deletions and t insertions (cost 2t) are replaced by at least g + t substitutions.  t is
    at most the smaller of the two runs, hence at most the second largest "d" / "i" run, hence below g: the shifted
    alignment costs more.  So the all-matching alignment is the only optimal one, and the rule's tuple, which is the
    tuple of SOME optimal alignment whatever its tie-breaking, is its tuple.  (Single edits with one kept token between
    them: the shift costs 2 as well, d is unchanged but the counts are no longer determined - hence two.)
    tests/test_edit_cpu.py checks the claim against ``rule`` at sizes up to 300; the GPU tests use it where the Python
    table would be too slow."""
    rng = np.random.default_rng(seed)
    used = sum(run for kind, run in sites if kind in "sd")
    slots = len(sites) + 1  # runs of kept tokens: before the first site, between sites, after the last
    di = sorted([run for kind, run in sites if kind in "di"] + [0, 0])
    g = max(2, 1 + di[-2])
    least = [0 if (k == 0 and first) or (k == slots - 1 and last) else g for k in range(slots)]
    spare = m - used - sum(least)
    open_slots = [k for k in range(slots) if not ((k == 0 and first) or (k == slots - 1 and last))]
    if spare < 0 or (spare > 0 and not open_slots):
        raise ValueError("the reference is too short for these sites (or, with one site at both ends, too long)")
    extra = np.zeros(slots, np.int64)
    if open_slots:
        cut = np.sort(rng.integers(0, spare + 1, len(open_slots) - 1))
        extra[open_slots] = np.diff(np.concatenate([[0], cut, [spare]]))
    ref = list(range(1000, 1000 + m))
    fresh = iter(range(100000, 100000 + 3 * 8192))
    hyp, pos, k = [], 0, {"s": 0, "d": 0, "i": 0}
    for slot in range(slots):
        keep = least[slot] + int(extra[slot])
        hyp += ref[pos:pos + keep]
        pos += keep
        if slot < len(sites):
            kind, run = sites[slot]
            k[kind] += run
            if kind in "si":
                hyp += [next(fresh) for _ in range(run)]
            if kind in "sd":
                pos += run
    assert pos == m
    return np.asarray(hyp, np.int32), np.asarray(ref, np.int32), (k["s"], k["d"], k["i"])


def planted_sizes(n, m, seed=0):
    """A planted pair with a hypothesis of exactly n and a reference of exactly m tokens: six sites, a substitution at the
    very first position and an insertion at the very end."""
    k_d, k_i = 2 + max(0, m - n), 2 + max(0, n - m)
    sites = [("s", 1), ("i", k_i - 1), ("d", 1), ("s", 2), ("d", k_d - 1), ("i", 1)]
    hyp, ref, k = planted_case(m, sites, seed, first=True, last=True)
    assert len(hyp) == n and len(ref) == m
    return hyp, ref, k
