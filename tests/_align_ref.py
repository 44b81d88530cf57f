"""Float64 references, seeded inputs and per-element bounds for the alignment kernels tmi_align_cost and tmi_dtw
(csrc/align.hip; the contracts are in include/tethys_mi.h).  CPU only: nothing here imports the GPU package, so
tests/test_align_cpu.py checks the references (against scipy, a plain double loop and a brute force over all paths), the
bounds (reachable by an honest fp32 restatement of each kernel, exceeded by every listed mutation) before
tests/test_align_kernels_gpu.py and tests/test_align_gpu.py compare the kernels with them.  tools/align_bench.py times
``cost_ref`` + ``dtw_ref`` as the host route.

Every bound is per element and analytic: a count of fp32 roundings times U = 2^-24 times magnitudes of the REFERENCE's
intermediates; gam(n) = n U / (1 - n U) bounds a chain of n roundings.  None is fitted, none is relative to a tensor-wide
maximum.

Cost (per item n with R = rows[n] tokens, per selected head, per frame t; p exact, being fp32 or bf16 input):
  mean   the fp32 sum of R values in any order and one division: e_mean = gam(R + 1) sum|p| / R       (R adds, 1 division)
  d      = fl(p - mean~): e_d = e_mean (1 + U) + U |d|                                                  (1 rounding)
  var    sum of R fma(d~, d~, .) and one division, all terms >= 0: relative gam(R + 1) on sum d~^2 / R, which differs
         from var by at most A = sum(2 |d| e_d + e_d^2) / R:  e_var = A + gam(R + 1) (var + A)
  rstd   x = fl(var~ + 1e-20f): rel_x = (e_var + U (var + 1e-20 + e_var) + U 1e-20) / (var + 1e-20)     (the add, the constant)
         rsqrtf within 2 ulp = 4 U (its documented 1 ulp, doubled): rel_r = (1 + rel_x / (2 (1 - rel_x))) (1 + 4U) - 1
  z      = fl(d~ rstd~): bound_z = (|d| + e_d) rstd (1 + rel_r) (1 + U) - |z|                           (1 rounding)
  median selects one of its inputs and is 1-Lipschitz in the largest perturbation of them: bound_m[s, t] = the largest
         bound_z inside the (reflected) window of (s, t).  No rounding of its own; a near-tie needs no special case.
  cost   acc = base (or 0), then one fma(-w_h, m_h, acc) per selected head, K of them:
         bound = sum_h |w_h| bound_m_h + gam(K) (|base| + sum_h |w_h| (|m_h| + bound_m_h))              (K roundings)
  normalize off: bound_z = 0, so one head of weight 1 onto nothing is exact.

DTW.  fp32 addition is monotone, so the kernel's D~ is the minimum over paths of the path's cost summed cell by cell in
fp32 (len - 1 additions after the first cell, which is added to 0 exactly): e(Q) = gam(len(Q) - 1) sum_{Q} |c|.  The traced
path P attains D~ (unless the tie c0 == c1 < c2 occurs on it, where the stated rule steps left, off the minimum), so with
P* the float64 optimum: cost64(P) - cost64(P*) <= e(P) + e(P*), and |total - cost64(P*)| <= max(e(P), e(P*)).  When the
costs themselves carry a bound b (the model-level test), sum_P b + sum_P* b is added, and |c| grows by b inside e.
"""
import numpy as np
import torch

from _row_kernel_ref import U, gam, guard_pattern, ratio  # noqa: F401  (shared with the kernel tests)

F32, BF16 = torch.float32, torch.bfloat16
VAR_EPS = 1e-20
FRAME_SECONDS = 0.02


# ------------------------------------------------------------------------------------------------------- median filter
def reflect_index(idx, cols):
    """-k -> k, cols-1+k -> cols-1-k (numpy pad "reflect"); needs |overhang| < cols."""
    idx = np.abs(idx)
    return np.where(idx > cols - 1, 2 * (cols - 1) - idx, idx)


def window_index(cols, width):
    """[cols, width] frame indices of every median window."""
    return reflect_index(np.arange(cols)[:, None] + np.arange(-(width // 2), width // 2 + 1)[None, :], cols)


def median_ref(z, width, variant=None):
    """Median of ``width`` along the last axis with reflected ends.  ``variant`` "edge": the end sample repeated (a mutation)."""
    cols = z.shape[-1]
    assert cols > width // 2
    if variant == "edge":
        idx = np.clip(np.arange(cols)[:, None] + np.arange(-(width // 2), width // 2 + 1)[None, :], 0, cols - 1)
    else:
        idx = window_index(cols, width)
    return np.median(z[..., idx], axis=-1)  # (odd width: the middle element itself)


# ----------------------------------------------------------------------------------------------------------------- cost
def cost_ref(p, rows, cols, head_weight, width, normalize, base=None, with_bound=True):
    """float64 cost and its per-element bound: p [N, H, S, T] float64 (values exact in the kernel's input dtype),
    head_weight float32 [H], base the fp32 cost accumulated onto (or None).  -> (cost, bound) [N, S, T], NaN where the
    kernel writes nothing.  ``with_bound=False``: the cost alone, (cost, None) - what a user aligning on the host computes."""
    p = np.asarray(p, dtype=np.float64)
    N, H, S, T = p.shape
    w = np.asarray(head_weight, dtype=np.float32).astype(np.float64)
    cost, bound = np.full((N, S, T), np.nan), np.full((N, S, T), np.nan)
    sel = [h for h in range(H) if w[h] != 0.0]
    for n in range(N):
        R, Cn = int(rows[n]), int(cols[n])
        idx = window_index(Cn, width)
        acc = np.zeros((R, Cn)) if base is None else np.asarray(base, dtype=np.float64)[n, :R, :Cn].copy()
        mag, berr = np.abs(acc), np.zeros((R, Cn))
        for h in sel:
            q = p[n, h, :R, :Cn]
            if normalize and not with_bound:
                d = q - q.mean(axis=0)
                z, bz = d / np.sqrt((d * d).mean(axis=0) + VAR_EPS), None
            elif normalize:
                mean = q.mean(axis=0)
                d = q - mean
                var = (d * d).mean(axis=0)
                x0 = var + VAR_EPS
                rstd = 1.0 / np.sqrt(x0)
                z = d * rstd
                e_mean = gam(R + 1) * np.abs(q).sum(axis=0) / R
                e_d = e_mean * (1 + U) + U * np.abs(d)
                A = (2 * np.abs(d) * e_d + e_d * e_d).sum(axis=0) / R
                e_var = A + gam(R + 1) * (var + A)
                rel_x = (e_var + U * (x0 + e_var) + U * VAR_EPS) / x0
                with np.errstate(divide="ignore", invalid="ignore"):
                    rel_r = np.where(rel_x < 1.0, (1 + rel_x / (2 * (1 - rel_x))) * (1 + 4 * U) - 1, np.inf)
                    bz = np.where(np.isfinite(rel_r), (np.abs(d) + e_d) * rstd * (1 + rel_r) * (1 + U) - np.abs(z), np.inf)
            else:
                z, bz = q, np.zeros_like(q)
            m = np.median(z[:, idx], axis=-1)
            acc = acc - w[h] * m
            if not with_bound:
                continue
            bm = bz[:, idx].max(axis=-1)
            berr = berr + abs(w[h]) * bm
            mag = mag + abs(w[h]) * (np.abs(m) + bm)
        cost[n, :R, :Cn] = acc
        bound[n, :R, :Cn] = berr + gam(len(sel)) * mag
    return cost, (bound if with_bound else None)


def _fold(part):
    a = part[0]
    for v in range(1, len(part)):
        a = a + part[v]
    return a


def cost_f32(p, rows, cols, head_weight, width, normalize, base=None, variant=None):
    """An fp32 numpy restatement of tmi_align_cost (sixteen interleaved partial sums, two-pass variance, fma by one rounding
    of the float64 value).  ``variant``: None, or a mutation - "sample_var" (/ (R - 1)), "edge" (repeated-end reflection)."""
    f = np.float32
    p = np.asarray(p, dtype=np.float64).astype(f)
    N, H, S, T = p.shape
    w = np.asarray(head_weight, dtype=f)
    out = np.full((N, S, T), np.nan, dtype=f)
    for n in range(N):
        R, Cn = int(rows[n]), int(cols[n])
        acc = np.zeros((R, Cn), dtype=f) if base is None else np.asarray(base, dtype=f)[n, :R, :Cn].copy()
        for h in range(H):
            if w[h] == 0:
                continue
            q = p[n, h, :R, :Cn]
            z = q
            if normalize:
                part = np.zeros((16, Cn), dtype=f)
                for s in range(R):
                    part[s % 16] = part[s % 16] + q[s]
                mean = _fold(part) / f(R)
                part = np.zeros((16, Cn), dtype=f)
                for s in range(R):
                    d = q[s] - mean
                    part[s % 16] = (d.astype(np.float64) * d.astype(np.float64) + part[s % 16].astype(np.float64)).astype(f)
                div = f(R - 1) if variant == "sample_var" else f(R)
                with np.errstate(divide="ignore", invalid="ignore"):
                    var = _fold(part) / div
                rstd = (1.0 / np.sqrt((var + f(VAR_EPS)).astype(np.float64))).astype(f)
                z = (q - mean) * rstd
            m = median_ref(z, width, "edge" if variant == "edge" else None).astype(f)
            acc = (-(w[h].astype(np.float64)) * m.astype(np.float64) + acc.astype(np.float64)).astype(f)
        out[n, :R, :Cn] = acc
    return out


def cost_inputs(N, H, S, T, dtype, seed, nan_head=None):
    """Attention-like weights: a softmax over the T frames of seeded logits with a drifting ridge (token s peaks near frame
    s T / S), rounded to ``dtype``; float64 values.  ``nan_head``: that head is all NaN (its weight must be 0)."""
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((N, H, S, T)) * 1.5
    centre = (np.arange(S)[:, None] + 0.5) * T / S
    logits -= 0.5 * ((np.arange(T)[None, :] - centre) / max(2.0, T / 8.0)) ** 2
    logits -= logits.max(axis=-1, keepdims=True)
    p = np.exp(logits)
    p /= p.sum(axis=-1, keepdims=True)
    p = torch.from_numpy(p).to(dtype).double().numpy()
    if nan_head is not None:
        p[:, nan_head] = np.nan
    return p


# ------------------------------------------------------------------------------------------------------------------ DTW
def dtw_tables(cost, dtype=np.float64, variant=None):
    """D and the moves of the stated recurrence over cost [R, C], one anti-diagonal at a time, in ``dtype`` (float32: the
    kernel's own arithmetic, bit for bit).  ``variant``: a mutation - "tie_diag" (ties take the diagonal), "no_up" (the
    upper predecessor dropped)."""
    c = np.asarray(cost).astype(dtype)
    R, Cn = c.shape
    D = np.full((R + 1, Cn + 1), np.inf, dtype=dtype)
    D[0, 0] = 0
    mv = np.zeros((R, Cn), dtype=np.uint8)
    for d in range(R + Cn - 1):
        i = np.arange(max(0, d - Cn + 1), min(R - 1, d) + 1)
        j = d - i
        c0, c1, c2 = D[i, j], D[i, j + 1], D[i + 1, j]
        if variant == "no_up":
            c1 = np.where(j == 0, c1, np.inf).astype(dtype)  # (the first column has nothing else)
        if variant == "tie_diag":
            m2 = (c2 < c0) & (c2 < c1)
            m1 = ~m2 & (c1 < c0) & (c1 < c2)
            mv[i, j] = np.where(m2, 2, np.where(m1, 1, 0))
        else:
            m0 = (c0 < c1) & (c0 < c2)
            m1 = ~m0 & (c1 < c0) & (c1 < c2)
            mv[i, j] = np.where(m0, 0, np.where(m1, 1, 2))
        D[i + 1, j + 1] = c[i, j] + np.minimum(c0, np.minimum(c1, c2))
    return D[1:, 1:], mv


def backtrace(mv):
    """The path [(i, j)] from (0, 0) to (R-1, C-1) that the moves trace back (first row: left, first column: up)."""
    i, j = mv.shape[0] - 1, mv.shape[1] - 1
    path = [(i, j)]
    while i > 0 or j > 0:
        m = 2 if i == 0 else (1 if j == 0 else int(mv[i, j]))
        if m == 0:
            i, j = i - 1, j - 1
        elif m == 1:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    return np.asarray(path[::-1], dtype=np.int64)


def token_bounds(path, R):
    """(start, end): the first frame of the path in each row and its last frame + 1."""
    start, end = np.full(R, np.iinfo(np.int64).max), np.full(R, -1)
    np.minimum.at(start, path[:, 0], path[:, 1])
    np.maximum.at(end, path[:, 0], path[:, 1] + 1)
    return start, end


def dtw_ref(cost, dtype=np.float64, variant=None):
    """-> {"path" [len, 2], "start", "end" [R], "total"} of cost [R, C]."""
    D, mv = dtw_tables(cost, dtype, variant)
    path = backtrace(mv)
    start, end = token_bounds(path, D.shape[0])
    return {"path": path, "start": start, "end": end, "total": D[-1, -1]}


def dtw_plain(cost):
    """The same recurrence as a plain double loop (float64): what dtw_tables is checked against."""
    R, Cn = cost.shape
    D = np.full((R + 1, Cn + 1), np.inf)
    D[0, 0] = 0.0
    mv = np.zeros((R, Cn), dtype=np.uint8)
    for i in range(R):
        for j in range(Cn):
            c0, c1, c2 = D[i, j], D[i, j + 1], D[i + 1, j]
            if c0 < c1 and c0 < c2:
                mv[i, j] = 0
            elif c1 < c0 and c1 < c2:
                mv[i, j] = 1
            else:
                mv[i, j] = 2
            D[i + 1, j + 1] = cost[i, j] + min(c0, c1, c2)
    return D[1:, 1:], mv


def all_paths(R, Cn):
    """Every monotone path from (0, 0) to (R-1, C-1) with steps (1, 1), (1, 0), (0, 1): small R, C only."""
    def walk(i, j):
        if i == R - 1 and j == Cn - 1:
            yield [(i, j)]
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < R and j + dj < Cn:
                for rest in walk(i + di, j + dj):
                    yield [(i, j)] + rest
    return list(walk(0, 0))


def path_cost(cost, path):
    return float(np.asarray(cost, dtype=np.float64)[path[:, 0], path[:, 1]].sum())


def path_problems(path, R, Cn, start=None, end=None):
    """What is wrong with a path for an R x C matrix (and with the token bounds reported next to it): [] when valid."""
    path = np.asarray(path)
    bad = []
    if path.ndim != 2 or path.shape[1] != 2 or len(path) < 1:
        return ["shape"]
    if tuple(path[0]) != (0, 0) or tuple(path[-1]) != (R - 1, Cn - 1):
        bad.append("end points")
    steps = {tuple(s) for s in np.diff(path, axis=0)}
    if not steps <= {(1, 1), (1, 0), (0, 1)}:
        bad.append(f"steps {sorted(steps)}")
    if not bad and start is not None:
        s, e = token_bounds(path, R)
        if not (np.array_equal(s, np.asarray(start)) and np.array_equal(e, np.asarray(end))):
            bad.append("token bounds")
    return bad


def path_err(cost, path, cell_bound=None):
    """e(Q) of the module docstring (+ the sum of the cells' own bounds)."""
    path = np.asarray(path)
    c = np.abs(np.asarray(cost, dtype=np.float64)[path[:, 0], path[:, 1]])
    b = 0.0 if cell_bound is None else np.asarray(cell_bound, dtype=np.float64)[path[:, 0], path[:, 1]]
    return float(gam(len(path) - 1) * (c + b).sum() + np.sum(b))


def dtw_bounds(cost, ref, path, cell_bound=None):
    """(excess bound, total bound): cost64(P) - cost64(P*) <= e(P) + e(P*), |total - cost64(P*)| <= max(e(P), e(P*))."""
    eP, eR = path_err(cost, path, cell_bound), path_err(cost, ref["path"], cell_bound)
    return eP + eR, max(eP, eR)


def grid_cost(R, Cn, seed):
    """Costs k / 64, |k| <= 1024: every fp32 sum over <= 1947 cells is exact (|sum| < 2^15, step 2^-6: 21 bits)."""
    return np.random.default_rng(seed).integers(-1024, 1025, size=(R, Cn)).astype(np.float64) / 64.0


def random_cost(R, Cn, seed):
    """fp32 costs shaped like the alignment's: minus a positive, heavy-tailed weight, a ridge along the diagonal."""
    rng = np.random.default_rng(seed)
    ridge = np.exp(-0.5 * ((np.arange(Cn)[None, :] - (np.arange(R)[:, None] + 0.5) * Cn / R) / max(2.0, Cn / 10.0)) ** 2)
    c = -(rng.gamma(2.0, 0.5, size=(R, Cn)) + 2.0 * ridge)
    return c.astype(np.float32).astype(np.float64)
