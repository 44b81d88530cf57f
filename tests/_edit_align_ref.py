"""Reference for tmi_edit_align and tmi_edit_confusion (include/tethys_mi.h, "Error-rate evaluation"): a plain Python
restatement of the table with its moves, of the trace, of the step triples with the caller's columns and of the confusion
fold, and a validity check of a path that needs no table.  No GPU, no torch."""
import itertools

import numpy as np

MATCH, SUB, DEL, INS = 0, 1, 2, 3
DIAG, UP, LEFT = 0, 1, 2
RULE = (DIAG, UP, LEFT)  # the header's order of the candidates


def normalise_cols(row, length=None, cols=None, stop_id=-1, skip_lo=0, skip_hi=0):
    """``_edit_ref.normalise`` with the columns: -> (kept tokens, their columns in ``row``)."""
    row = [int(x) for x in row]
    cols = len(row) if cols is None else int(cols)
    length = cols if length is None else int(length)
    row = row[:max(0, min(length, cols))]
    if stop_id != -1 and stop_id in row:
        row = row[:row.index(stop_id)]
    kept = [(x, c) for c, x in enumerate(row) if not (skip_lo <= x < skip_hi)]
    return [x for x, _ in kept], [c for _, c in kept]


def moves(h, r, order=RULE):
    """(d, move) of every cell: d[i][j] the distance of h[:i] and r[:j], move[i][j] the candidate that won - the candidates
    are tried in ``order`` and a later one replaces an earlier one only when its d is strictly smaller.  Row 0 moves left,
    column 0 moves up (move[0][0] is unused)."""
    n, m = len(h), len(r)
    d = [list(range(m + 1))] + [[i] + [0] * m for i in range(1, n + 1)]
    mv = [bytearray([LEFT] * (m + 1))] + [bytearray([UP] + [0] * m) for _ in range(n)]
    for i in range(1, n + 1):
        di, dp, mi, hi = d[i], d[i - 1], mv[i], h[i - 1]
        for j in range(1, m + 1):
            cand = (dp[j - 1] + (hi != r[j - 1]), dp[j] + 1, di[j - 1] + 1)
            best = order[0]
            for c in order[1:]:
                if cand[c] < cand[best]:
                    best = c
            di[j], mi[j] = cand[best], best
    return d, mv


def trace(h, r, mv):
    """The path from (n, m) back to (0, 0) through ``mv``, in forward order: [(op, i, j)] with i / j the positions in the
    kept rows h / r, -1 for the missing side."""
    i, j, path = len(h), len(r), []
    while i > 0 or j > 0:
        move = LEFT if i == 0 else UP if j == 0 else mv[i][j]
        if move == DIAG:
            i, j = i - 1, j - 1
            path.append((SUB if h[i] != r[j] else MATCH, i, j))
        elif move == UP:
            i -= 1
            path.append((INS, i, -1))
        else:
            j -= 1
            path.append((DEL, -1, j))
    return path[::-1]


def align(h, r, order=RULE):
    """-> (out, path): out = (d, sub, del, ins, n, m) counted along the path of ``trace``."""
    d, mv = moves(h, r, order)
    path = trace(h, r, mv)
    k = [sum(1 for op, _, _ in path if op == o) for o in (SUB, DEL, INS)]
    assert sum(k) == d[len(h)][len(r)]
    return (sum(k), k[0], k[1], k[2], len(h), len(r)), path


def reference(hyp, ref, hyp_len=None, ref_len=None, R=1, stop_id=-1, skip=(0, 0), hyp_cols=None, ref_cols=None):
    """What tmi_edit_align writes: (out int32 [N, 6], steps: a list of N lists of (op, hyp column, ref column), n_steps
    int32 [N]); pair i = hypothesis i against reference i // R."""
    hyp, ref = np.asarray(hyp), np.asarray(ref)
    N = hyp.shape[0]
    out, steps, n_steps = np.zeros((N, 6), np.int32), [], np.zeros(N, np.int32)
    refs = [normalise_cols(ref[b], None if ref_len is None else ref_len[b], ref.shape[1] if ref_cols is None else ref_cols,
                           stop_id, skip[0], skip[1]) for b in range(ref.shape[0])]
    for i in range(N):
        h, hc = normalise_cols(hyp[i], None if hyp_len is None else hyp_len[i], hyp.shape[1] if hyp_cols is None else hyp_cols,
                               stop_id, skip[0], skip[1])
        r, rc = refs[i // R]
        out[i], path = align(h, r)
        steps.append([(op, hc[a] if a >= 0 else -1, rc[b] if b >= 0 else -1) for op, a, b in path])
        n_steps[i] = len(path)
    return out, steps, n_steps


def confusion(steps, hyp, ref, V, R=1, first_only=True):
    """What tmi_edit_confusion writes (from zero): int64 [(V + 1) * (V + 1) + 1]; ``steps`` as ``reference`` returns them."""
    counts = np.zeros((V + 1) * (V + 1) + 1, np.int64)
    for i, st in enumerate(steps):
        if first_only and i % R:
            continue
        for op, a, b in st:
            row = V if op == INS else int(ref[i // R][b])
            col = V if op == DEL else int(hyp[i][a])
            ok = (op == INS or 0 <= row < V) and (op == DEL or 0 <= col < V)
            counts[row * (V + 1) + col if ok else -1] += 1
    return counts


def check_path(h_row, r_row, steps, out, h_len=None, r_len=None, stop_id=-1, skip=(0, 0)):
    """"" when ``steps`` [(op, hyp column, ref column)] is a valid alignment of the two rows that agrees with ``out``, else
    what is wrong with it.  No table: the columns of each side must be strictly increasing and be exactly the columns of
    the kept tokens, every op must agree with the equality of the two tokens it names, the numbers of ops 1, 2, 3 must
    be out[1..3] and the number of non-match steps out[0].  A valid path with as many edits as the Levenshtein distance
    is an optimal one."""
    h, hc = normalise_cols(h_row, h_len, None, stop_id, skip[0], skip[1])
    r, rc = normalise_cols(r_row, r_len, None, stop_id, skip[0], skip[1])
    steps = [tuple(int(x) for x in s) for s in steps]
    for k, (op, a, b) in enumerate(steps):
        if op not in (MATCH, SUB, DEL, INS):
            return f"step {k}: op {op}"
        if (a == -1) != (op == DEL) or (b == -1) != (op == INS):
            return f"step {k}: op {op} with columns ({a}, {b})"
    if [a for _, a, _ in steps if a != -1] != hc:  # (hc is strictly increasing: so are they)
        return "the hypothesis columns are not the kept tokens' columns in order"
    if [b for _, _, b in steps if b != -1] != rc:
        return "the reference columns are not the kept tokens' columns in order"
    for k, (op, a, b) in enumerate(steps):
        if op in (MATCH, SUB) and (int(h_row[a]) == int(r_row[b])) != (op == MATCH):
            return f"step {k}: op {op} on tokens {int(h_row[a])}, {int(r_row[b])}"
    k = [sum(1 for op, _, _ in steps if op == o) for o in (SUB, DEL, INS)]
    if k != [int(x) for x in out[1:4]] or sum(k) != int(out[0]):
        return f"the op counts {k} are not out = {[int(x) for x in out[:4]]}"
    if (int(out[4]), int(out[5])) != (len(h), len(r)):
        return f"out has n, m = {int(out[4])}, {int(out[5])} for {len(h)}, {len(r)} kept tokens"
    return ""


def exhaustive_pairs(symbols=(0, 1), longest=4):
    """Every pair of strings over ``symbols`` of length 0 .. longest as two padded int32 arrays with their lengths: 961
    pairs for the defaults."""
    seqs = [list(t) for k in range(longest + 1) for t in itertools.product(symbols, repeat=k)]
    pairs = [(h, r) for h in seqs for r in seqs]
    hyp = np.full((len(pairs), max(longest, 1)), -7, np.int32)
    ref = np.full((len(pairs), max(longest, 1)), -9, np.int32)
    hl, rl = np.zeros(len(pairs), np.int32), np.zeros(len(pairs), np.int32)
    for i, (h, r) in enumerate(pairs):
        hyp[i, :len(h)], ref[i, :len(r)], hl[i], rl[i] = h, r, len(h), len(r)
    return hyp, ref, hl, rl
