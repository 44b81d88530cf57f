"""tmi_align_cost and tmi_dtw (csrc/align.hip) through the C ABI, against the float64 references and the per-element bounds
of tests/_align_ref.py (checked by tests/test_align_cpu.py).

Every input and output lies inside a larger buffer of 7.0 / NaN guards (integers: 7 / a large negative) with padded
strides, compared bit for bit after the call wherever the contract says nothing is written: the guard zones, the stride
padding, the rows past rows[n] and the frames past cols[n].  Measured / bound goes through ``_margins.within`` under the
names "align ..." with the bound 1; no bound is fitted to what the kernels give.

DTW, exact cases: costs on the grid k / 64, |k| <= 1024, so every fp32 sum over <= 1947 cells is exact and the path, the
token bounds and the total must EQUAL the reference, ties included.  Random cases: a valid path whose float64 cost is
within e(P) + e(P*) of the optimum (module docstring of _align_ref.py)."""
import numpy as np
import pytest
import torch

import _align_ref as A
from _margins import within

pytestmark = pytest.mark.gpu

F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
TMI_ERR_INVALID = -1
PAD = 64


def _L():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib as L
    return L


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class G:
    """``n`` payload elements inside guards; ``v`` is the payload on the device."""

    def __init__(self, dev, dtype, n, data=None):
        host = A.guard_pattern(n + 2 * PAD, dtype)
        if data is not None:
            host[PAD:PAD + n] = data
        self.host0, self.t, self.n = host.clone(), host.to(dev), n
        self.v = self.t[PAD:PAD + n]

    def now(self):
        return self.t.cpu()

    def same_where(self, keep):
        """The guard zones and every payload element with ``keep`` set are bit for bit what they were."""
        full = torch.ones(self.n + 2 * PAD, dtype=torch.bool)
        full[PAD:PAD + self.n] = keep.reshape(-1)
        return torch.equal(bits(self.now())[full], bits(self.host0)[full])


def stream():
    return torch.cuda.current_stream().cuda_stream


def dt_code(dtype):
    return _L().TMI_BF16 if dtype == BF16 else _L().TMI_F32


# ======================================================================================================= tmi_dtw
def run_dtw(dev, costs, S_max=None, T_max=None, c_ss=None, c_sn=None, want_path=True):
    """costs: a list of [rows, cols] float64 matrices (fp32-exact) -> the raw outputs and the guard verdict."""
    lib = _L().lib()
    N = len(costs)
    S_max = S_max or max(c.shape[0] for c in costs)
    T_max = T_max or max(c.shape[1] for c in costs)
    c_ss = c_ss or T_max
    c_sn = c_sn or S_max * c_ss
    host = A.guard_pattern(N * c_sn, F32)
    for n, c in enumerate(costs):
        R, Cn = c.shape
        view = host[n * c_sn:n * c_sn + S_max * c_ss].view(S_max, c_ss)
        view[:R, :Cn] = torch.from_numpy(c).float()
    cost = G(dev, F32, N * c_sn, host)
    rows = torch.tensor([c.shape[0] for c in costs], dtype=I32, device=dev)
    cols = torch.tensor([c.shape[1] for c in costs], dtype=I32, device=dev)
    ts, te = G(dev, I32, N * S_max), G(dev, I32, N * S_max)
    tot = G(dev, F32, N)
    P = S_max + T_max - 1
    path, plen = G(dev, I32, N * P * 2), G(dev, I32, N)
    ws_bytes = lib.tmi_dtw_workspace_bytes(N, S_max, T_max)
    assert ws_bytes > 0
    ws = G(dev, I32, ws_bytes // 4)
    rc = lib.tmi_dtw(cost.v.data_ptr(), c_sn, c_ss, rows.data_ptr(), cols.data_ptr(), N, S_max, T_max, ts.v.data_ptr(),
                     te.v.data_ptr(), tot.v.data_ptr(), path.v.data_ptr() if want_path else None,
                     plen.v.data_ptr() if want_path else None, ws.v.data_ptr(), ws_bytes, stream())
    assert rc == 0, lib.tmi_last_error()
    torch.cuda.synchronize()
    out = {"start": ts.now()[PAD:-PAD].view(N, S_max), "end": te.now()[PAD:-PAD].view(N, S_max), "total": tot.now()[PAD:-PAD],
           "path": path.now()[PAD:-PAD].view(N, P, 2), "len": plen.now()[PAD:-PAD]}
    # nothing outside the contract is written: the cost is read-only, the workspace stays inside its bytes
    assert cost.same_where(torch.ones(N * c_sn, dtype=torch.bool)), "cost was written"
    assert ws.same_where(torch.zeros(ws.n, dtype=torch.bool)), "workspace guards"
    keep_tok = torch.ones(N, S_max, dtype=torch.bool)
    keep_path = torch.ones(N, P, 2, dtype=torch.bool)
    for n, c in enumerate(costs):
        keep_tok[n, :c.shape[0]] = False
        if want_path:
            keep_path[n, :int(out["len"][n])] = False
    assert ts.same_where(keep_tok) and te.same_where(keep_tok), "token bounds past rows[n]"
    assert tot.same_where(torch.zeros(N, dtype=torch.bool)), "total guards"
    assert path.same_where(keep_path), "path past path_len[n]"
    assert plen.same_where(torch.full((N,), not want_path, dtype=torch.bool)), "path_len"
    return out


def check_exact(out, n, c):
    R, Cn = c.shape
    ref = A.dtw_ref(c)
    L = int(out["len"][n])
    got = out["path"][n, :L].numpy().astype(np.int64)
    assert L == len(ref["path"]) and np.array_equal(got, ref["path"]), (R, Cn)
    assert np.array_equal(out["start"][n, :R].numpy(), ref["start"]) and np.array_equal(out["end"][n, :R].numpy(), ref["end"])
    assert float(out["total"][n]) == float(ref["total"])


EXACT = [(1, 1), (1, 7), (5, 1), (2, 2), (63, 40), (64, 40), (65, 40), (129, 200), (448, 1500)]


@pytest.mark.parametrize("shape", EXACT, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dtw_exact(dev, shape):
    c = A.grid_cost(*shape, seed=shape[0] * 7 + shape[1])
    check_exact(run_dtw(dev, [c]), 0, c)


def test_dtw_exact_many_ties(dev):
    """Costs on a coarse grid (k / 8, |k| <= 16): most comparisons tie; and the all-zero matrix of the tie rule."""
    c = np.round(A.grid_cost(70, 90, seed=5) / 8)
    z = np.zeros((66, 20))
    out = run_dtw(dev, [c, z])
    check_exact(out, 0, c)
    check_exact(out, 1, z)
    assert [tuple(x) for x in out["path"][1, :int(out["len"][1])].tolist()] == [(i, 0) for i in range(66)] + [(65, j) for j in range(1, 20)]


def test_dtw_exact_ragged_in_one_launch(dev):
    """N = 3 items of different sizes inside S_max = 70, T_max = 100, with a padded row stride and item stride."""
    cs = [A.grid_cost(70, 33, 1), A.grid_cost(1, 100, 2), A.grid_cost(65, 97, 3)]
    out = run_dtw(dev, cs, S_max=70, T_max=100, c_ss=107, c_sn=70 * 107 + 13)
    for n, c in enumerate(cs):
        check_exact(out, n, c)
    out = run_dtw(dev, cs, S_max=70, T_max=100, c_ss=107, c_sn=70 * 107 + 13, want_path=False)  # path == NULL
    for n, c in enumerate(cs):
        ref = A.dtw_ref(c)
        assert np.array_equal(out["start"][n, :c.shape[0]].numpy(), ref["start"]) and float(out["total"][n]) == float(ref["total"])


@pytest.mark.parametrize("shape", [(65, 300), (448, 1500)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_dtw_random(dev, shape):
    R, Cn = shape
    c = A.random_cost(R, Cn, seed=R)
    out = run_dtw(dev, [c])
    L = int(out["len"][0])
    path = out["path"][0, :L].numpy().astype(np.int64)
    assert A.path_problems(path, R, Cn, out["start"][0, :R].numpy(), out["end"][0, :R].numpy()) == []
    ref = A.dtw_ref(c)
    excess_bound, total_bound = A.dtw_bounds(c, ref, path)
    excess = A.path_cost(c, path) - ref["total"]
    print(f"align dtw random {R}x{Cn}: excess {excess:.3e} of {excess_bound:.3e}, total off by "
          f"{abs(float(out['total'][0]) - ref['total']):.3e} of {total_bound:.3e}")
    assert excess >= -1e-9 * abs(ref["total"])
    within(f"align dtw random {R}x{Cn} excess", max(excess, 0.0) / excess_bound, 1.0)
    within(f"align dtw random {R}x{Cn} total", abs(float(out["total"][0]) - ref["total"]) / total_bound, 1.0)
    # and, being the same fp32 arithmetic, the fp32 restatement's answer bit for bit
    r32 = A.dtw_ref(c, np.float32)
    assert np.array_equal(path, r32["path"]) and float(out["total"][0]) == float(r32["total"])


def test_dtw_twice_is_bit_identical(dev):
    c = A.random_cost(130, 410, seed=9)
    a, b = run_dtw(dev, [c, c[:77, :200]]), run_dtw(dev, [c, c[:77, :200]])
    for k in ("start", "end", "total", "path", "len"):
        assert torch.equal(bits(a[k]), bits(b[k])), k


def test_dtw_invalid_arguments(dev):
    lib = _L().lib()
    N, S, T = 2, 8, 16
    cost = torch.zeros(N, S, T, device=dev)
    rows = torch.full((N,), S, dtype=I32, device=dev)
    cols = torch.full((N,), T, dtype=I32, device=dev)
    ts, te = G(dev, I32, N * S), G(dev, I32, N * S)
    tot, path, plen = G(dev, F32, N), G(dev, I32, N * (S + T - 1) * 2), G(dev, I32, N)
    nbytes = lib.tmi_dtw_workspace_bytes(N, S, T)
    ws = torch.zeros(nbytes // 4, dtype=I32, device=dev)
    good = dict(cost=cost.data_ptr(), c_sn=S * T, c_ss=T, rows=rows.data_ptr(), cols=cols.data_ptr(), N=N, S=S, T=T,
                ts=ts.v.data_ptr(), te=te.v.data_ptr(), tot=tot.v.data_ptr(), path=path.v.data_ptr(), plen=plen.v.data_ptr(),
                ws=ws.data_ptr(), nbytes=nbytes)
    order = ("cost", "c_sn", "c_ss", "rows", "cols", "N", "S", "T", "ts", "te", "tot", "path", "plen", "ws", "nbytes")
    bad = [dict(cost=None), dict(rows=None), dict(cols=None), dict(ts=None), dict(te=None), dict(tot=None), dict(ws=None),
           dict(path=None), dict(plen=None), dict(N=0), dict(S=0), dict(T=0), dict(S=1025), dict(T=4097), dict(c_ss=T - 1),
           dict(c_sn=S * T - 1), dict(nbytes=nbytes - 1), dict(cost=cost.data_ptr() + 2)]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        assert lib.tmi_dtw(*[a[k] for k in order], stream()) == TMI_ERR_INVALID, kw
        assert b"tmi_dtw" in lib.tmi_last_error()
    torch.cuda.synchronize()
    for g in (ts, te, tot, path, plen):  # nothing was launched
        assert g.same_where(torch.ones(g.n, dtype=torch.bool))


# ================================================================================================ tmi_align_cost
_REF = {}


def cost_case(name, N, H, S, T, rows, cols, dtype, width, normalize, hw, nan_head=None, seed=0):
    key = (name, dtype, width, normalize)
    if key not in _REF:
        p = A.cost_inputs(N, H, S, T, dtype, seed + 17 * width, nan_head)
        ref, bound = A.cost_ref(p, rows, cols, hw, width, normalize)
        _REF[key] = (p, ref, bound)
    return _REF[key]


def run_cost(dev, p, rows, cols, hw, dtype, width, normalize, accumulate=False, base=None, p_pad=5, c_pad=3):
    """p float64 [N, H, S, T] -> the fp32 cost [N, S, T] as the kernel left it (guards where it wrote nothing)."""
    lib = _L().lib()
    N, H, S, T = p.shape
    p_sq, c_ss = T + p_pad, T + c_pad
    p_sbh, c_sn = S * p_sq + 2 * p_pad, S * c_ss + 7
    ph = A.guard_pattern(N * H * p_sbh, dtype)
    for n in range(N):
        for h in range(H):
            o = (n * H + h) * p_sbh
            ph[o:o + S * p_sq].view(S, p_sq)[:, :T] = torch.from_numpy(p[n, h]).to(dtype)
    P = G(dev, dtype, N * H * p_sbh, ph)
    ch = A.guard_pattern(N * c_sn, F32)
    if base is not None:
        for n in range(N):
            ch[n * c_sn:n * c_sn + S * c_ss].view(S, c_ss)[:, :T] = base[n]
    Cst = G(dev, F32, N * c_sn, ch)
    rows_d = torch.tensor(rows, dtype=I32, device=dev)
    cols_d = torch.tensor(cols, dtype=I32, device=dev)
    hw_d = torch.from_numpy(np.asarray(hw, dtype=np.float32)).to(dev)
    rc = lib.tmi_align_cost(P.v.data_ptr(), dt_code(dtype), p_sbh, p_sq, rows_d.data_ptr(), cols_d.data_ptr(), hw_d.data_ptr(),
                            Cst.v.data_ptr(), c_sn, c_ss, N, H, S, T, width, int(normalize), int(accumulate), stream())
    assert rc == 0, lib.tmi_last_error()
    torch.cuda.synchronize()
    assert P.same_where(torch.ones(P.n, dtype=torch.bool)), "the weights were written"
    keep = torch.ones(N * c_sn, dtype=torch.bool)
    for n in range(N):
        keep[n * c_sn:n * c_sn + S * c_ss].view(S, c_ss)[:rows[n], :cols[n]] = False
    assert Cst.same_where(keep), "cost written outside rows[n] x cols[n]"
    now = Cst.now()[PAD:-PAD]
    return torch.stack([now[n * c_sn:n * c_sn + S * c_ss].view(S, c_ss)[:, :T] for n in range(N)])


def compare_cost(name, got, ref, bound, rows, cols):
    worst = 0.0
    for n in range(len(rows)):
        R, Cn = rows[n], cols[n]
        worst = max(worst, A.ratio(got[n, :R, :Cn], torch.from_numpy(ref[n, :R, :Cn]), torch.from_numpy(bound[n, :R, :Cn])))
        if R == 1:
            assert bool((got[n, :1, :Cn] == 0).all()) or not name.startswith("norm"), "one token must give exactly 0"
    print(f"align cost {name}: {worst:.3f} of its bound")
    within(f"align cost {name}", worst, 1.0)


HW3 = [0.5, 0.0, 0.5]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("width", [1, 3, 7])
@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
def test_cost_ragged(dev, dtype, width, normalize):
    """N = 3 ragged items, H = 3 with a zero-weight head full of NaN, padded strides; cols: two tiles + 3, one above the
    tile, 4; rows 17, 2, 1."""
    tile = int(_L().lib().tmi_align_cost_tile(width))
    T = 2 * tile + 3
    rows, cols = [17, 2, 1], [T, tile + 1, 4]
    p, ref, bound = cost_case("ragged", 3, 3, 17, T, rows, cols, dtype, width, normalize, HW3, nan_head=1, seed=1)
    got = run_cost(dev, p, rows, cols, HW3, dtype, width, normalize)
    assert not bool(torch.isnan(torch.cat([got[n, :rows[n], :cols[n]].reshape(-1) for n in range(3)])).any()), "the NaN head was read"
    compare_cost(f"{'norm' if normalize else 'raw'} ragged w{width} {'bf16' if dtype == BF16 else 'fp32'}", got, ref, bound, rows, cols)
    again = run_cost(dev, p, rows, cols, HW3, dtype, width, normalize)
    assert torch.equal(bits(got), bits(again)), "two calls differ"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("width", [1, 3, 7])
def test_cost_tile_edges(dev, dtype, width):
    """cols one below and equal to the frame tile (and rows 17, 2)."""
    tile = int(_L().lib().tmi_align_cost_tile(width))
    rows, cols = [17, 2], [tile - 1, tile]
    p, ref, bound = cost_case("edges", 2, 2, 17, tile, rows, cols, dtype, width, True, [0.25, 0.75], seed=2)
    got = run_cost(dev, p, rows, cols, [0.25, 0.75], dtype, width, True)
    compare_cost(f"norm edges w{width} {'bf16' if dtype == BF16 else 'fp32'}", got, ref, bound, rows, cols)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_cost_full_size(dev, dtype):
    """rows 448, cols 1500: max_target_positions x n_ctx."""
    rows, cols = [448], [1500]
    p, ref, bound = cost_case("full", 1, 3, 448, 1500, rows, cols, dtype, 7, True, HW3, nan_head=1, seed=3)
    got = run_cost(dev, p, rows, cols, HW3, dtype, 7, True, p_pad=4, c_pad=4)
    compare_cost(f"norm 448x1500 w7 {'bf16' if dtype == BF16 else 'fp32'}", got, ref, bound, rows, cols)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_cost_one_head_raw_is_exact(dev, dtype):
    """normalize off, width 7, one head of weight 1: the cost is minus the median, exactly."""
    tile = int(_L().lib().tmi_align_cost_tile(7))
    T = 2 * tile + 3
    rows, cols = [17, 5], [T, tile + 1]
    p = A.cost_inputs(2, 1, 17, T, dtype, 8)
    ref, _ = A.cost_ref(p, rows, cols, [1.0], 7, False)
    got = run_cost(dev, p, rows, cols, [1.0], dtype, 7, False)
    for n in range(2):
        assert np.array_equal(got[n, :rows[n], :cols[n]].double().numpy(), ref[n, :rows[n], :cols[n]])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_cost_accumulate_over_two_calls(dev, dtype):
    tile = int(_L().lib().tmi_align_cost_tile(7))
    T = tile + 9
    rows, cols = [17, 3], [T, 30]
    p1, p2 = A.cost_inputs(2, 3, 17, T, dtype, 21, nan_head=1), A.cost_inputs(2, 3, 17, T, dtype, 22, nan_head=1)
    first = run_cost(dev, p1, rows, cols, HW3, dtype, 7, True)
    base = torch.nan_to_num(first, nan=0.0)  # (outside rows x cols the buffer holds guards either way)
    got = run_cost(dev, p2, rows, cols, HW3, dtype, 7, True, accumulate=True, base=[first[n] for n in range(2)])
    ref, bound = A.cost_ref(p2, rows, cols, HW3, 7, True, base=base.double().numpy())
    compare_cost(f"norm accumulate w7 {'bf16' if dtype == BF16 else 'fp32'}", got, ref, bound, rows, cols)
    ref0, _ = A.cost_ref(p2, rows, cols, HW3, 7, True)
    assert float(np.nanmax(np.abs(ref - ref0))) > 0.1  # (the first call's cost is really in the result)


def test_cost_invalid_arguments(dev):
    lib = _L().lib()
    N, H, S, T = 2, 2, 4, 40
    p = torch.zeros(N, H, S, T, device=dev)
    cost = G(dev, F32, N * S * T)
    rows = torch.full((N,), S, dtype=I32, device=dev)
    cols = torch.full((N,), T, dtype=I32, device=dev)
    hw = torch.ones(H, device=dev)
    good = dict(p=p.data_ptr(), dt=0, p_sbh=S * T, p_sq=T, rows=rows.data_ptr(), cols=cols.data_ptr(), hw=hw.data_ptr(),
                cost=cost.v.data_ptr(), c_sn=S * T, c_ss=T, N=N, H=H, S=S, T=T, w=7, norm=1, acc=0)
    order = ("p", "dt", "p_sbh", "p_sq", "rows", "cols", "hw", "cost", "c_sn", "c_ss", "N", "H", "S", "T", "w", "norm", "acc")
    bad = [dict(p=None), dict(rows=None), dict(cols=None), dict(hw=None), dict(cost=None), dict(dt=2), dict(p_sq=T - 1),
           dict(p_sbh=S * T - 1), dict(c_ss=T - 1), dict(c_sn=S * T - 1), dict(N=0), dict(H=0), dict(H=33), dict(S=0), dict(T=0),
           dict(w=0), dict(w=2), dict(w=11), dict(w=9, T=4, p_sq=4, c_ss=4), dict(norm=2), dict(acc=-1),
           dict(p=p.data_ptr() + 2), dict(cost=cost.v.data_ptr() + 1)]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        assert lib.tmi_align_cost(*[a[k] for k in order], stream()) == TMI_ERR_INVALID, kw
        assert b"tmi_align_cost" in lib.tmi_last_error()
    torch.cuda.synchronize()
    assert cost.same_where(torch.ones(cost.n, dtype=torch.bool))  # nothing was launched
