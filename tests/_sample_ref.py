"""tmi_lm_head_sample's choice rule (include/tethys_mi.h) restated in numpy, fp64, with the integer part taken from
oracle.dropout.  Besides the token and its log-probability every row reports whether it is DECIDED: whether the same
token comes out for every score vector within ``b`` of the given one and every fp32 evaluation of the rule.  A kernel
must match the decided rows exactly; an undecided row is one whose draw sits on an edge.

Margins at b = 0 cover the kernel's fp32 arithmetic only, and are about twice what is measured.  ``P_TOL``, relative to
the candidates' mass, has two parts: ``P_SUM_TOL`` for s - lse, exp and the running sum in fp32 given lse
(``running_sum_error_fp32``: 1.6e-6 on the exact-score inputs, recorded by test_sample_cpu.py), and ``P_LP_TOL`` for
the kernel's own lse, which moves every p_i by the same factor: the absolute error of its log-probabilities (1.4e-6 on those inputs,
recorded by test_sample_gpu.py's exact-score test).  ``G_TOL``, absolute on each perturbed score s + g of the Gumbel rule:
``gumbel_error_fp32`` measures 1.5e-6 on the same inputs (half an ulp of s + g < 16 and a few ulp of -log(-log u))."""
import numpy as np

from oracle import dropout as D

P_SUM_TOL = 3.2e-6
P_LP_TOL = 3e-6
P_TOL = P_SUM_TOL + P_LP_TOL
G_TOL = 3e-6  # on each of the two perturbed scores compared
KMAX = 64


def sample_bits(seed, rows, cols):
    """tmi_sample_bits(tmi_row_key(tmi_stream_key(seed, 0), row), col) over the broadcast of ``rows`` and ``cols``."""
    ra, rb = D.row_key(D.stream_key(seed, 0), np.asarray(rows, dtype=np.uint64))
    c = np.asarray(cols, dtype=np.uint64) & D.M32
    return D.mix32(ra ^ D.mix32(c ^ rb))


def uniform(bits):
    return ((np.asarray(bits, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def step_seed(seed, t):
    return (int(seed) + t * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def rank(s, suppress_id=-1):
    """s [M, V] fp64 scores (already divided by the temperature) -> (s with the suppressed column at -inf, lse [M], the
    KMAX + 1 best columns per row [M, KMAX + 1], best first, the smaller column first among equals)."""
    s = np.array(s, dtype=np.float64)
    if suppress_id >= 0:
        s[:, suppress_id] = -np.inf
    mx = s.max(axis=1)
    lse = mx + np.log(np.exp(s - mx[:, None]).sum(axis=1))
    n = min(KMAX + 1, s.shape[1])
    top = np.argsort(-s, axis=1, kind="stable")[:, :n]
    return s, lse, top


def choose_topk(s, lse, top, seed, top_k, top_p, b=0.0, rows=None):
    """-> token [M], logprob [M], decided [M] (bool), allowed [M, top_k + 1] (the columns an undecided row may still
    give: the reference's top-(k + 1))."""
    M, V = s.shape
    rows = np.arange(M) if rows is None else np.asarray(rows)
    b_rows = np.broadcast_to(np.asarray(b, dtype=np.float64), (M,))
    token, logprob, decided = np.zeros(M, np.int64), np.zeros(M), np.zeros(M, bool)
    u = uniform(sample_bits(seed, rows, 0xFFFFFFFF))
    for r in range(M):
        sc = s[r, top[r]]
        b = float(b_rows[r])
        rel = 2.0 * np.expm1(2.0 * b) + P_TOL
        k = int(min(top_k, np.isfinite(sc).sum(), V))
        p = np.exp(sc[:k] - lse[r])
        P = np.cumsum(p)
        ok = True
        if k < len(sc) and np.isfinite(sc[k]):
            ok &= sc[k - 1] - sc[k] > 2 * b or b == 0.0  # (b = 0: equal scores keep their column order, the rule's own)
        if top_p < 1.0:
            m = int(np.argmax(P >= top_p * P[-1])) + 1
            ok &= bool(np.all(np.abs(P - top_p * P[-1]) > rel * P[-1]))
        else:
            m = k
        thr = u[r] * P[m - 1]
        hit = np.nonzero(P[:m] > thr)[0]
        j = int(hit[0]) if len(hit) else m - 1
        ok &= bool(np.all(np.abs(P[:m] - thr) > rel * P[m - 1]))
        if j > 0:
            ok &= sc[j - 1] - sc[j] > 2 * b or b == 0.0  # (b = 0: equal scores keep their column order)
        if j + 1 < k:
            ok &= sc[j] - sc[j + 1] > 2 * b or b == 0.0
        token[r], logprob[r], decided[r] = top[r, j], sc[j] - lse[r], ok
    return token, logprob, decided, top[:, :top_k + 1]


def choose_gumbel(s, lse, seed, b=0.0, rows=None):
    """-> token [M], logprob [M], decided [M], runner_up [M]."""
    M, V = s.shape
    rows = np.arange(M) if rows is None else np.asarray(rows)
    u = uniform(sample_bits(seed, rows[:, None], np.arange(V)[None, :]))
    pert = s + -np.log(-np.log(u))
    order = np.argsort(-pert, axis=1, kind="stable")[:, :2]
    tok = order[:, 0]
    ar = np.arange(M)
    best = pert[ar, tok]
    second = pert[ar, order[:, 1]] if V > 1 else np.full(M, -np.inf)
    b = np.broadcast_to(np.asarray(b, dtype=np.float64), (M,))
    return tok, s[ar, tok] - lse, best - second > 2 * b + 2 * G_TOL, order[:, 1] if V > 1 else tok


# ----------------------------------------------------------------------------- the inputs of tests/test_sample_gpu.py
# Built on the host, so that the undecided-row caps can be checked from the restatement alone (tests/test_sample_cpu.py)
# for the very seeds the GPU tests use.  A seed bump below moves one configuration off an edge of its running sums; it
# is chosen from the restatement, never from a kernel's output.
V, VP = 51865, 51904
EXACT_MS, EXACT_TS = (1, 5, 16, 17, 40), (0.5, 1.0, 2.0)
EXACT_KP = tuple((k, p) for k in (1, 2, 50, 64) for p in (1.0, 0.9, 0.3)) + ((0, 1.0),)  # (0: Gumbel mode)
EXACT_CAP = 0.01
_EXACT_BUMP = {}
_EXACT_INPUT = {16: 200}  # M -> generator seed of its inputs (default 100 + M): a nucleus edge does not move with the draw's seed
_EXACT = {}


def exact_seed(M, T, top_k, top_p):
    return 1000 * M + int(T * 10) + 100000 * _EXACT_BUMP.get((M, T, top_k, top_p), 0)


def exact_inputs(M):
    """x in {-1, 0, 1} [M, 128], w multiples of 1/8 in [-1/2, 1/2] [128, VP] (zero pad columns): every partial sum of a score
    is a multiple of 1/8 below 2^7, exact in fp32 and bf16 in any order, and T in {0.5, 1, 2} keeps z / T exact.
    -> x, w (float32), z [M, V] (fp64), scale [M] = max_n sum_k |x_k w_kn|."""
    if M not in _EXACT:
        rng = np.random.RandomState(_EXACT_INPUT.get(M, 100 + M))
        x = rng.randint(-1, 2, size=(M, 128)).astype(np.float32)
        w = np.zeros((128, VP), dtype=np.float32)
        w[:, :V] = rng.randint(-4, 5, size=(128, V)) / 8.0
        z = x.astype(np.float64) @ w[:, :V].astype(np.float64)
        scale = (np.abs(x.astype(np.float64)) @ np.abs(w[:, :V].astype(np.float64))).max(1)
        _EXACT[M] = (x, w, z, scale, {})
    return _EXACT[M][:4]


def exact_ranked(M, T):
    exact_inputs(M)
    z, cache = _EXACT[M][2], _EXACT[M][4]
    if T not in cache:
        cache[T] = rank(z / T)
    return cache[T]


def exact_choice(M, T, top_k, top_p):
    """-> token, logprob, decided, allowed ([M, n] columns an undecided row may give) of one configuration, at b = 0."""
    s, lse, top = exact_ranked(M, T)
    seed = exact_seed(M, T, top_k, top_p)
    if top_k:
        return choose_topk(s, lse, top, seed, top_k, top_p)
    tok, lp, dec, second = choose_gumbel(s, lse, seed)
    return tok, lp, dec, np.stack([tok, second], 1)


def cap_ok(decided, cap):
    """At most ``cap`` of a configuration's rows undecided."""
    return int((~decided).sum()) <= cap * len(decided)


RANDOM_DS, RANDOM_MS, RANDOM_T, RANDOM_CAP = (128, 768, 1280), (5, 17), 0.7, 0.10
RANDOM_KP = ((50, 0.9), (64, 1.0), (2, 0.3), (10, 1.0), (0, 1.0))
REL = 3e-7  # test_lm_head_topk_matches_fp64's: |s - s64| and |lse - lse64| <= REL * (scale + |lse|)
_RANDOM_BUMP = {}
_RANDOM_INPUT = {1280: 4000}  # d -> generator seed of its inputs (default 2100 + d)
_RANDOM = {}


def random_seed(wdt, d, M, top_k, top_p):
    return 7 * d + M + 31 * top_k + 1000 * _RANDOM_BUMP.get((wdt, d, M, top_k, top_p), 0)


def random_inputs(wdt, d):
    """test_lm_head_topk_matches_fp64's inputs from a host generator: w [d, VP] (bf16 or fp32, zero pad columns), gamma,
    beta, and per M the activations [3 M, d] of which the rows 2, 5, 8, ... are decoded (torch CPU tensors); and per M
    the fp64 reference (s, lse, top, b) with b = REL * (scale + |lse|)."""
    import torch
    g = torch.Generator().manual_seed(_RANDOM_INPUT.get(d, 2100 + d))
    w = torch.zeros(d, VP)
    w[:, :V] = torch.randn(d, V, generator=g) * d ** -0.5
    dt = torch.bfloat16 if wdt == "bf16" else torch.float32
    w = w.to(dt)
    gamma = 1 + 0.1 * torch.randn(d, generator=g)
    beta = 0.1 * torch.randn(d, generator=g)
    xs = {M: (torch.randn(M * 3, d, generator=g) * 2 + 0.5).to(dt) for M in RANDOM_MS}
    if (wdt, d) not in _RANDOM:
        wd = w[:, :V].double()
        refs = {}
        for M, full in xs.items():
            y = full[2::3].double()
            mu = y.mean(1, keepdim=True)
            var = ((y - mu) ** 2).mean(1, keepdim=True)
            y = (y - mu) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double()
            s, lse, top = rank(((y @ wd) / RANDOM_T).numpy())
            scale = ((y.abs() @ wd.abs()).max(1).values / RANDOM_T).numpy()
            refs[M] = (s, lse, top, REL * (scale + np.abs(lse)))
        _RANDOM[(wdt, d)] = refs
    return w, gamma, beta, xs, _RANDOM[(wdt, d)]


def random_choice(ref, wdt, d, M, top_k, top_p):
    s, lse, top, b = ref
    seed = random_seed(wdt, d, M, top_k, top_p)
    if top_k:
        return choose_topk(s, lse, top, seed, top_k, top_p, b=b)
    tok, lp, dec, second = choose_gumbel(s, lse, seed, b=b)
    return tok, lp, dec, np.stack([tok, second], 1)


# ----------------------------------------------------------------------------- the margins, measured
def running_sum_error_fp32(s, lse, top, top_k):
    """max_j |P_j(fp32) - P_j(fp64)| / P_{k-1} per row, the rule's arithmetic after lse done in fp32 as the kernel does it:
    s - lse, exp and the running sum in index order, each rounded to fp32 (lse itself given in fp32)."""
    M = s.shape[0]
    out = np.zeros(M)
    for r in range(M):
        sc = s[r, top[r, :top_k]]
        P64 = np.cumsum(np.exp(sc - lse[r]))
        p32 = np.exp((sc.astype(np.float32) - np.float32(lse[r])).astype(np.float32)).astype(np.float32)
        P32 = np.zeros(len(p32), np.float32)
        acc = np.float32(0)
        for j, v in enumerate(p32):
            acc = np.float32(acc + v)
            P32[j] = acc
        out[r] = np.abs(P32.astype(np.float64) - P64).max() / P64[-1]
    return out


def gumbel_error_fp32(s, seed):
    """max_n |(s + g)(fp32) - (s + g)(fp64)| per row over the columns within 40 of the row's best (the others cannot win),
    with -log u taken the kernel's way (1 - u from 2^23 up) and every step rounded to fp32."""
    M, Vn = s.shape
    n = (sample_bits(seed, np.arange(M)[:, None], np.arange(Vn)[None, :]) >> np.uint64(8)).astype(np.int64)
    u64 = (n + 0.5) * 2.0 ** -24
    p64 = s + -np.log(-np.log(u64))
    f = np.float32
    lo = (n.astype(f) + f(0.5)) * f(2.0 ** -24)
    hi = ((0xFFFFFF - n).astype(f) + f(0.5)) * f(2.0 ** -24)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(n < (1 << 23), -np.log(lo, dtype=f), -np.log1p(-hi, dtype=f)).astype(f)
        p32 = (s.astype(f) + (-np.log(e, dtype=f))).astype(f)
    near = p64 >= p64.max(1, keepdims=True) - 40
    return np.where(near, np.abs(p32.astype(np.float64) - p64), 0.0).max(1)
