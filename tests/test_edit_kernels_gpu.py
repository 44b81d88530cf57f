"""tmi_edit_distance (csrc/edit.hip) through ``ops.edit_distance`` and through the C ABI, against tests/_edit_ref.py (checked
by tests/test_edit_cpu.py).  The outputs are integers: every element of ``out`` is compared for equality.

Random tier: a 4-symbol alphabet (ties in every cell) with the kept lengths n, m over {0, 1, 2, 63, 64, 65, 255, 256, 257},
all 81 combinations, compared with the Python table.  Planted tier: sizes up to the limit 4096 x 4096, where the Python
table is too slow, against the counts the pair was built with (``planted_case`` gives the argument)."""
import numpy as np
import pytest
import torch

import _edit_ref as E

pytestmark = pytest.mark.gpu

I32 = torch.int32
TMI_ERR_INVALID = -1
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257)
GARBAGE = 0x5A5A5A5A


def _mods():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops
    return _lib, ops


def stream():
    return torch.cuda.current_stream().cuda_stream


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def run(dev, hyp, ref, hyp_len=None, ref_len=None, hyp_cols=None, ref_cols=None, **kw):
    """``ops.edit_distance`` on the first hyp_cols / ref_cols columns of the host rows (the rest is stride padding)."""
    _, ops = _mods()
    h, r = dv(hyp, dev), dv(ref, dev)
    h = h if hyp_cols is None else h[:, :hyp_cols]
    r = r if ref_cols is None else r[:, :ref_cols]
    out = ops.edit_distance(h, r, None if hyp_len is None else dv(hyp_len, dev), None if ref_len is None else dv(ref_len, dev), **kw)
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def grid():
    """All 81 (n, m) combinations, one pair each: rows of 260 columns in a buffer of 263, garbage past every length."""
    rng = np.random.default_rng(2301)
    pairs = [(n, m) for m in LENGTHS for n in LENGTHS]
    hyp = E.random_rows(rng, [p[0] for p in pairs], 260, ld=263)
    ref = E.random_rows(rng, [p[1] for p in pairs], 260, ld=261)
    hl, rl = np.asarray([p[0] for p in pairs], np.int32), np.asarray([p[1] for p in pairs], np.int32)
    want = E.reference(hyp, ref, hl, rl, hyp_cols=260, ref_cols=260)
    return hyp, ref, hl, rl, want, pairs


def test_random_grid_all_81_length_combinations(dev, grid):
    hyp, ref, hl, rl, want, pairs = grid
    got = run(dev, hyp, ref, hl, rl, hyp_cols=260, ref_cols=260)
    assert want[:, 4:].tolist() == [list(p) for p in pairs]
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, [(pairs[i], got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    assert (got[:, 1] + got[:, 2] + got[:, 3] == got[:, 0]).all() and (got[:, 3] - got[:, 2] == got[:, 4] - got[:, 5]).all()


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("Nr", [1, 5, 17])
def test_random_n_best_layout_with_stop_and_skip(dev, R, Nr):
    """N = Nr * R hypotheses against Nr references: raw rows with skip-range tokens mixed in, a stop token in every second
    row with symbols after it, lengths above the column count and below zero, garbage past the length."""
    rng = np.random.default_rng(100 * R + Nr)
    lens = [0, 1, 2, 31, 63, 64, 65, 90]

    def side(rows, cols):
        buf = E.random_rows(rng, [0] * rows, cols, ld=cols + 5)
        ln = np.zeros(rows, np.int32)
        for i in range(rows):
            n = int(rng.choice(lens))
            sym = rng.integers(0, 4, n + 8)
            raw = E.sprinkle(rng, sym, n + (8 if i % 2 else 0), stop_at=n if i % 2 else None)[:cols]
            buf[i, :len(raw)] = raw
            ln[i] = len(raw)
        ln[0] = cols + 7 if rows > 1 else ln[0]  # above the column count: the row is its `cols` columns
        if rows > 2:
            ln[2] = -3                           # negative: empty
        return buf, ln

    hyp, hl = side(Nr * R, 200)
    ref, rl = side(Nr, 180)
    kw = dict(R=R, stop_id=E.STOP, skip=E.SKIP)
    want = E.reference(hyp, ref, hl, rl, hyp_cols=200, ref_cols=180, **kw)
    got = run(dev, hyp, ref, hl, rl, hyp_cols=200, ref_cols=180, **kw)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    # without lengths every row is its columns, the garbage included (it is only compared)
    want = E.reference(hyp, ref, R=R, hyp_cols=200, ref_cols=180)
    got = run(dev, hyp, ref, hyp_cols=200, ref_cols=180, R=R)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n,m", [(1023, 1025), (4096, 511), (511, 4096), (4096, 4096)])
def test_planted_counts_up_to_the_limit(dev, n, m):
    hyp, ref, (ks, kd, ki) = E.planted_sizes(n, m, seed=n + m)
    got = run(dev, hyp[None, :], ref[None, :])
    assert got.tolist() == [[ks + kd + ki, ks, kd, ki, n, m]]


@pytest.mark.parametrize("n,m", [(4096, 4096), (4096, 1000), (700, 4096), (1, 4096)])
def test_identical_and_disjoint_rows(dev, n, m):
    a = np.arange(10, 10 + n, dtype=np.int32)
    b = np.arange(10, 10 + m, dtype=np.int32)
    c = np.arange(50000, 50000 + m, dtype=np.int32)
    k = min(n, m)
    # one row is a prefix of the other: the shorter one matches, the rest is inserted or deleted
    assert run(dev, a[None, :], b[None, :]).tolist() == [[max(n, m) - k, 0, max(m - n, 0), max(n - m, 0), n, m]]
    if n == m:
        assert run(dev, a[None, :], a[None, :]).tolist() == [[0, 0, 0, 0, n, n]]
    assert run(dev, a[None, :], c[None, :]).tolist() == [[max(n, m), k, max(m - n, 0), max(n - m, 0), n, m]]


def test_compaction_across_wave_and_workgroup_boundaries(dev):
    """Skipped tokens straddling the 64- and 256-element boundaries, a whole wave's worth of skipped tokens, and the stop at
    63, 64 and 256: the kept tokens must arrive in order whichever lanes and waves held them."""
    rng = np.random.default_rng(7)
    cols = 600
    rows, lens = [], []

    def add(row):
        rows.append(row + [0] * (cols - len(row)))
        lens.append(len(row))

    base = [int(x) for x in rng.integers(0, 4, cols)]
    for lo, hi in ((60, 68), (250, 262), (64, 128), (0, 64), (63, 65), (255, 257), (128, 320)):
        add([100 + (k % 10) if lo <= k < hi else base[k] for k in range(cols)])
    for stop in (0, 63, 64, 256):
        row = list(base)
        row[stop] = E.STOP
        if stop + 9 < cols:
            row[stop + 9] = E.STOP  # (a later stop changes nothing)
        add(row)
    add([100 + (k % 10) for k in range(cols)])           # everything skipped
    add([100 if k % 2 else base[k] for k in range(cols)])  # every second token skipped
    hyp = np.asarray(rows, np.int32)
    ref = np.asarray([base[200:240]], np.int32).repeat(len(rows), 0)
    kw = dict(stop_id=E.STOP, skip=E.SKIP)
    hl = np.asarray(lens, np.int32)
    want = E.reference(hyp, ref, hl, **kw)
    assert np.array_equal(run(dev, hyp, ref, hl, **kw), want)
    # and with the roles exchanged (the reference side is compacted by the same code, on a workgroup of its own width)
    want = E.reference(ref, hyp, None, hl, **kw)
    assert np.array_equal(run(dev, ref, hyp, None, hl, **kw), want)


def test_two_calls_equal_bits_and_nothing_else_is_written(dev, grid):
    _, ops = _mods()
    hyp, ref, hl, rl, want, _ = grid
    N = hyp.shape[0]
    h, r, hlen, rlen = dv(hyp, dev)[:, :260], dv(ref, dev)[:, :260], dv(hl, dev), dv(rl, dev)
    bufs = []
    for _ in range(2):
        buf = torch.full((N + 1, 8), GARBAGE, dtype=I32, device=dev)
        ret = ops.edit_distance(h, r, hlen, rlen, out=buf[:N])
        assert ret.data_ptr() == buf.data_ptr()
        bufs.append(buf.cpu().numpy())
    assert np.array_equal(bufs[0], bufs[1])
    assert np.array_equal(bufs[0][:N, :6], want)
    assert (bufs[0][:N, 6:] == GARBAGE).all() and (bufs[0][N] == GARBAGE).all()


def test_refusals_write_nothing_and_the_limits_pass(dev):
    L, _ = _mods()
    lib = L.lib()
    hyp = torch.zeros(4, 4100, dtype=I32, device=dev)
    ref = torch.zeros(4, 4100, dtype=I32, device=dev)
    ln = torch.full((4,), 3, dtype=I32, device=dev)
    out = torch.full((5, 8), GARBAGE, dtype=I32, device=dev)
    good = dict(hyp=hyp.data_ptr(), hyp_ld=4100, hyp_cols=16, hyp_len=ln.data_ptr(), ref=ref.data_ptr(), ref_ld=4100, ref_cols=16,
                ref_len=ln.data_ptr(), N=4, R=1, stop=-1, lo=0, hi=0, out=out.data_ptr(), out_ld=8)

    def call(**over):
        a = dict(good, **over)
        return lib.tmi_edit_distance(a["hyp"], a["hyp_ld"], a["hyp_cols"], a["hyp_len"], a["ref"], a["ref_ld"], a["ref_cols"],
                                     a["ref_len"], a["N"], a["R"], a["stop"], a["lo"], a["hi"], a["out"], a["out_ld"], stream())

    bad = [dict(hyp=None), dict(ref=None), dict(out=None), dict(hyp_cols=4097, hyp_ld=4100), dict(ref_cols=4097), dict(N=0),
           dict(N=65536), dict(R=3), dict(R=0), dict(hyp_ld=15), dict(ref_ld=15), dict(out_ld=5), dict(hyp_cols=-1),
           dict(hyp=hyp.data_ptr() + 2), dict(ref=ref.data_ptr() + 1), dict(out=out.data_ptr() + 2), dict(hyp_len=ln.data_ptr() + 2),
           dict(ref_len=ln.data_ptr() + 1)]
    for over in bad:
        assert call(**over) == TMI_ERR_INVALID, over
        assert lib.tmi_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GARBAGE).all()
    # the limits themselves: 4096 columns on both sides, R == N, no lengths
    assert call(hyp_cols=4096, ref_cols=4096, hyp_len=None, ref_len=None, R=4, ref_ld=4100) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[:4, :6].tolist() == [[0, 0, 0, 0, 4096, 4096]] * 4 and (got[:4, 6:] == GARBAGE).all() and (got[4] == GARBAGE).all()


def test_wrapper_checks_on_the_host(dev):
    _, ops = _mods()
    h = torch.zeros(6, 8, dtype=I32, device=dev)
    r = torch.zeros(2, 8, dtype=I32, device=dev)
    assert ops.edit_distance(h, r, R=3).shape == (6, 6)
    assert ops.edit_distance(h[:, 2:], r[:, 1:5], R=3).cpu().numpy()[:, 4:].tolist() == [[6, 4]] * 6  # strided views, no copy
    for args, kw in (((h.long(), r), {}), ((h.cpu(), r), {}), ((h, r), dict(R=2)), ((h, r[0]), {}), ((h[:, ::2], r), dict(R=3)),
                     ((h, r), dict(R=3, hyp_len=torch.zeros(5, dtype=I32, device=dev))),
                     ((h, r), dict(R=3, ref_len=torch.zeros(2, dtype=torch.int64, device=dev))),
                     ((torch.zeros(1, 4097, dtype=I32, device=dev), r[:1]), {})):
        with pytest.raises((ValueError, TypeError)):
            ops.edit_distance(*args, **kw)
