"""tmi_edit_align and tmi_edit_confusion (csrc/edit.hip) through the C ABI and through ``ops``, against
tests/_edit_align_ref.py (checked by tests/test_edit_align_cpu.py).  Every output is an integer and is compared for equality.

Every launch of this file goes through ``align``: the outputs, a guard band behind each of them and the workspace are
filled with a sentinel first; afterwards the guard bands and every step at or past n_steps must still hold it, and ``out``
must equal ``ops.edit_distance`` on the same arguments."""
import numpy as np
import pytest
import torch

import _edit_align_ref as A
import _edit_ref as E

pytestmark = pytest.mark.gpu

I32 = torch.int32
TMI_ERR_INVALID = -1
GARBAGE = 0x5A5A5A5A
GUARD = 64  # int32 entries behind steps, n_steps and the workspace


def _mods():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops
    return _lib, ops


def stream():
    return torch.cuda.current_stream().cuda_stream


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def align(dev, hyp, ref, hyp_len=None, ref_len=None, R=1, stop_id=-1, skip=(0, 0), ws_fill=GARBAGE, raw=False):
    """One tmi_edit_align launch on device tensors (views are fine) -> (out [N, 6], steps: N lists of triples, n_steps [N]) as
    numpy / lists; ``raw``: (the three whole buffers with their guard bands, the workspace) as numpy instead."""
    L, ops = _mods()
    N, hc = hyp.shape
    rc = ref.shape[1]
    S = hc + rc
    ws_elems = ops.edit_align_workspace_elems(N, hc, rc)
    out = torch.full((N * 6 + GUARD,), GARBAGE, dtype=I32, device=dev)
    steps = torch.full((N * 3 * S + GUARD,), GARBAGE, dtype=I32, device=dev)
    n_steps = torch.full((N + GUARD,), GARBAGE, dtype=I32, device=dev)
    ws = torch.full((ws_elems + GUARD,), ws_fill, dtype=I32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    rc_ = L.lib().tmi_edit_align(hyp.data_ptr(), hyp.stride(0) if N > 1 else max(hc, 1), hc, p(hyp_len), ref.data_ptr(),
                                 ref.stride(0) if ref.shape[0] > 1 else max(rc, 1), rc, p(ref_len), N, R, stop_id, skip[0], skip[1],
                                 out.data_ptr(), 6, steps.data_ptr(), 3 * S, n_steps.data_ptr(), ws.data_ptr(), ws_elems * 4, stream())
    assert rc_ == 0, L.lib().tmi_last_error()
    torch.cuda.synchronize()
    o, s, ns, w = out.cpu().numpy(), steps.cpu().numpy(), n_steps.cpu().numpy(), ws.cpu().numpy()
    assert (o[N * 6:] == GARBAGE).all() and (s[N * 3 * S:] == GARBAGE).all() and (ns[N:] == GARBAGE).all()
    assert (w[ws_elems:] == ws_fill).all()
    if raw:
        return o, s, ns, w
    o, s, ns = o[:N * 6].reshape(N, 6), s[:N * 3 * S].reshape(N, S, 3), ns[:N]
    assert (ns >= 0).all() and (ns <= S).all()
    for i in range(N):
        assert (s[i, ns[i]:] == GARBAGE).all(), f"pair {i}: steps at or past n_steps = {ns[i]} were written"
    dist = ops.edit_distance(hyp, ref, hyp_len, ref_len, R=R, stop_id=stop_id, skip=skip).cpu().numpy()
    assert np.array_equal(o, dist), "out differs from tmi_edit_distance"
    return o, [[tuple(int(x) for x in t) for t in s[i, :ns[i]]] for i in range(N)], ns


def against_reference(dev, hyp, ref, hyp_len=None, ref_len=None, hyp_cols=None, ref_cols=None, **kw):
    """Host rows -> the launch on their first hyp_cols / ref_cols columns (the rest is stride padding) equals the reference."""
    h, r = dv(hyp, dev), dv(ref, dev)
    h = h if hyp_cols is None else h[:, :hyp_cols]
    r = r if ref_cols is None else r[:, :ref_cols]
    got = align(dev, h, r, None if hyp_len is None else dv(hyp_len, dev), None if ref_len is None else dv(ref_len, dev), **kw)
    want = A.reference(hyp, ref, hyp_len, ref_len, hyp_cols=hyp_cols, ref_cols=ref_cols, **kw)
    assert np.array_equal(got[0], want[0]), (got[0].tolist(), want[0].tolist())
    assert np.array_equal(got[2], want[2])
    bad = [i for i in range(len(want[1])) if got[1][i] != want[1][i]]
    assert not bad, (bad[:5], got[1][bad[0]][:12], want[1][bad[0]][:12])
    return got


# ------------------------------------------------------------------------------------------------- exhaustive and boundary shapes
def test_exhaustive_pairs_over_two_symbols_in_one_launch(dev):
    hyp, ref, hl, rl = A.exhaustive_pairs()
    assert hyp.shape[0] == 961
    against_reference(dev, hyp, ref, hl, rl)


@pytest.mark.parametrize("hc,rc,N", [(1, 1, 3), (15, 17, 3), (16, 16, 3), (17, 15, 3), (63, 65, 3), (64, 64, 3), (65, 63, 3),
                                      (70, 1100, 1), (1100, 70, 1), (300, 200, 2), (448, 448, 8)])
def test_boundary_shapes_against_the_full_reference(dev, hc, rc, N):
    """Random rows over 4 symbols (ties in every cell) that fill their columns: one wave, two waves, the edges of the 64-cell
    move words, more reference columns than the workgroup has threads, the CTC and the Whisper shape."""
    rng = np.random.default_rng(1000 * hc + rc)
    hyp = E.random_rows(rng, [hc] * N, hc, ld=hc + 3)
    ref = E.random_rows(rng, [rc] * N, rc, ld=rc + 1)
    if N > 1:  # one pair with shorter rows inside the same columns
        hyp[1, hc // 2:], ref[1, (2 * rc) // 3:] = 7, 8
    hl = np.asarray([hc] * N, np.int32)
    rl = np.asarray([rc] * N, np.int32)
    if N > 1:
        hl[1], rl[1] = hc // 2, (2 * rc) // 3
    against_reference(dev, hyp, ref, hl, rl, hyp_cols=hc, ref_cols=rc)


# ------------------------------------------------------------------------------------------------- edge cases of the call
def test_empty_sides_lengths_and_the_stop_in_the_first_column(dev):
    rng = np.random.default_rng(3)
    hyp = E.random_rows(rng, [9] * 8, 9, ld=12)
    ref = E.random_rows(rng, [7] * 8, 7, ld=9)
    hl = np.asarray([0, 5, 0, -3, 99, 9, 4, 9], np.int32)   # n = 0; m = 0; both; a negative length; one above the columns
    rl = np.asarray([6, 0, 0, 7, 99, -3, 7, 3], np.int32)
    hyp[6, 0] = E.STOP                                       # the stop in the first column: an empty hypothesis
    ref[7, 0] = E.STOP
    o, steps, ns = against_reference(dev, hyp, ref, hl, rl, hyp_cols=9, ref_cols=7, stop_id=E.STOP)
    assert ns.tolist()[:4] == [6, 5, 0, 7] and o[4, 4:].tolist() == [9, 7] and ns[6] == 7 and ns[7] == 9
    assert steps[0] == [(A.DEL, -1, c) for c in range(6)] and steps[1] == [(A.INS, c, -1) for c in range(5)] and steps[2] == []


def test_skip_ranges_report_the_original_columns(dev):
    hyp = np.asarray([[1, 105, 2, 101, 101, 3, 0, 0], [100, 101, 102, 103, 104, 105, 106, 107], [1, 2, 3, 4, 5, 6, 7, 8]], np.int32)
    ref = np.asarray([[109, 1, 2, 100, 3, 3], [1, 2, 3, 1, 2, 3], [100, 100, 100, 101, 101, 101]], np.int32)
    hl = np.asarray([6, 8, 8], np.int32)
    o, steps, ns = against_reference(dev, hyp, ref, hl, None, skip=E.SKIP)
    # pair 0: 1 2 3 against 1 2 3 3 - the columns are those of the rows as passed, not of the compacted ones
    assert steps[0] == [(A.MATCH, 0, 1), (A.MATCH, 2, 2), (A.DEL, -1, 4), (A.MATCH, 5, 5)]
    assert ns.tolist() == [4, 6, 8] and o[1].tolist() == [6, 0, 6, 0, 0, 6] and o[2].tolist() == [8, 0, 0, 8, 8, 0]


def test_n_best_layout_strided_views_and_extreme_tokens(dev):
    """R = 3 hypotheses a reference, both sides views ``t[:, 2:]`` of wider tensors, raw rows with skip-range tokens and stop
    tokens mixed in, and the tokens -1 and 2^31 - 1 as ordinary symbols."""
    rng = np.random.default_rng(17)
    Nr, R, hc, rc = 5, 3, 90, 80

    def side(rows, cols):
        buf = E.random_rows(rng, [0] * rows, cols + 2, ld=cols + 5)
        ln = np.zeros(rows, np.int32)
        for i in range(rows):
            n = int(rng.choice([0, 1, 2, 31, 40, 63]))
            raw = E.sprinkle(rng, rng.integers(0, 4, n + 8), n + (8 if i % 2 else 0), stop_at=n if i % 2 else None)[:cols]
            buf[i, 2:2 + len(raw)] = raw
            ln[i] = len(raw)
        return buf, ln

    hyp, hl = side(Nr * R, hc)
    ref, rl = side(Nr, rc)
    hyp[4, 2:12] = [-1, 2 ** 31 - 1, -1, -1, 2 ** 31 - 1, 0, 1, -1, 2 ** 31 - 1, 2 ** 31 - 1]
    ref[1, 2:10] = [2 ** 31 - 1, -1, -1, 2 ** 31 - 1, 1, -1, 2 ** 31 - 1, 0]
    hl[4], rl[1] = 10, 8
    kw = dict(R=R, stop_id=E.STOP, skip=E.SKIP)
    got = align(dev, dv(hyp, dev)[:, 2:2 + hc], dv(ref, dev)[:, 2:2 + rc], dv(hl, dev), dv(rl, dev), **kw)
    want = A.reference(hyp[:, 2:], ref[:, 2:], hl, rl, hyp_cols=hc, ref_cols=rc, **kw)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and got[1] == want[1]
    # without lengths every row is its columns, the garbage behind the symbols included (it is only compared)
    got = align(dev, dv(hyp, dev)[:, 2:2 + hc], dv(ref, dev)[:, 2:2 + rc], R=R)
    want = A.reference(hyp[:, 2:], ref[:, 2:], R=R, hyp_cols=hc, ref_cols=rc)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]


# ------------------------------------------------------------------------------------------------- the limit
def test_planted_pair_at_the_limit(dev):
    hyp, ref, (ks, kd, ki) = E.planted_sizes(4096, 4096, seed=5)
    o, steps, ns = align(dev, dv(hyp[None, :], dev), dv(ref[None, :], dev))
    assert o.tolist() == [[ks + kd + ki, ks, kd, ki, 4096, 4096]] and ns.tolist() == [4096 + ki]
    assert A.check_path(hyp, ref, steps[0], o[0]) == ""
    # every kept token is aligned with its own copy (``planted_case`` says why no other optimal alignment exists)
    assert sum(1 for op, _, _ in steps[0] if op == A.MATCH) == 4096 - ks - kd


def test_random_pair_at_the_limit_is_a_valid_optimal_path(dev):
    rng = np.random.default_rng(4096)
    hyp, ref = rng.integers(0, 4, (1, 4096)).astype(np.int32), rng.integers(0, 4, (1, 4096)).astype(np.int32)
    o, steps, ns = align(dev, dv(hyp, dev), dv(ref, dev))  # (out == tmi_edit_distance is checked inside)
    assert A.check_path(hyp[0], ref[0], steps[0], o[0]) == ""
    assert ns[0] == 4096 + o[0, 3] == 4096 + o[0, 2]


# ------------------------------------------------------------------------------------------------- reproducibility, refusals
def test_two_calls_equal_bits_whatever_the_workspace_holds(dev):
    rng = np.random.default_rng(23)
    hyp, ref = dv(E.random_rows(rng, [130] * 6, 130), dev), dv(E.random_rows(rng, [97] * 2, 97), dev)
    runs = [align(dev, hyp, ref, R=3, ws_fill=fill, raw=True) for fill in (GARBAGE, GARBAGE, -1, 0)]
    for other in runs[1:]:
        for a, b in zip(runs[0][:3], other[:3]):
            assert np.array_equal(a, b)
    assert np.array_equal(runs[0][3], runs[1][3])  # the same call leaves the same workspace, too


def test_refusals_write_nothing_and_the_limits_pass(dev):
    L, ops = _mods()
    lib = L.lib()
    hyp = torch.zeros(4, 4100, dtype=I32, device=dev)
    ref = torch.zeros(4, 4100, dtype=I32, device=dev)
    ln = torch.full((4,), 3, dtype=I32, device=dev)
    out = torch.full((5, 8), GARBAGE, dtype=I32, device=dev)
    steps = torch.full((4, 3 * 8192 + 4), GARBAGE, dtype=I32, device=dev)
    n_steps = torch.full((8,), GARBAGE, dtype=I32, device=dev)
    need = lib.tmi_edit_align_workspace_bytes(4, 16, 16)
    assert need == 4 * 33 * 1 * 16 and lib.tmi_edit_align_workspace_bytes(1, 4096, 4096) == 8193 * 65 * 16
    ws = torch.full((need // 4 + 8,), GARBAGE, dtype=I32, device=dev)
    good = dict(hyp=hyp.data_ptr(), hyp_ld=4100, hyp_cols=16, hyp_len=ln.data_ptr(), ref=ref.data_ptr(), ref_ld=4100, ref_cols=16,
                ref_len=ln.data_ptr(), N=4, R=1, stop=-1, lo=0, hi=0, out=out.data_ptr(), out_ld=8, steps=steps.data_ptr(),
                steps_ld=steps.stride(0), n_steps=n_steps.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)

    def call(**over):
        a = dict(good, **over)
        return lib.tmi_edit_align(a["hyp"], a["hyp_ld"], a["hyp_cols"], a["hyp_len"], a["ref"], a["ref_ld"], a["ref_cols"],
                                  a["ref_len"], a["N"], a["R"], a["stop"], a["lo"], a["hi"], a["out"], a["out_ld"], a["steps"],
                                  a["steps_ld"], a["n_steps"], a["ws"], a["ws_bytes"], stream())

    bad = [dict(hyp=None), dict(ref=None), dict(out=None), dict(hyp_cols=4097, hyp_ld=4100), dict(ref_cols=4097), dict(N=0),
           dict(N=65536), dict(R=3), dict(R=0), dict(hyp_ld=15), dict(ref_ld=15), dict(out_ld=5), dict(hyp_cols=-1),
           dict(hyp=hyp.data_ptr() + 2), dict(ref=ref.data_ptr() + 1), dict(out=out.data_ptr() + 2), dict(hyp_len=ln.data_ptr() + 2),
           dict(ref_len=ln.data_ptr() + 1),
           dict(steps=None), dict(n_steps=None), dict(ws=None), dict(steps=steps.data_ptr() + 2), dict(n_steps=n_steps.data_ptr() + 1),
           dict(ws=ws.data_ptr() + 2), dict(steps_ld=3 * 32 - 1), dict(ws_bytes=need - 1), dict(ws_bytes=0)]
    for over in bad:
        assert call(**over) == TMI_ERR_INVALID, over
        assert lib.tmi_last_error()
    for N, hc, rc in ((0, 4, 4), (65536, 4, 4), (1, 4097, 4), (1, 4, 4097), (1, -1, 4)):
        assert lib.tmi_edit_align_workspace_bytes(N, hc, rc) == -1
        with pytest.raises(ValueError):
            ops.edit_align_workspace_elems(N, hc, rc)
    torch.cuda.synchronize()
    for t in (out, steps, n_steps, ws):
        assert (t.cpu().numpy() == GARBAGE).all()
    # the smallest strides and sizes pass: steps_ld = 3 (hyp_cols + ref_cols), the workspace to the byte
    assert call(steps_ld=3 * 32, N=1) == 0
    torch.cuda.synchronize()
    assert n_steps.cpu().numpy().tolist() == [3] + [GARBAGE] * 7 and out.cpu().numpy()[0, :6].tolist() == [0, 0, 0, 0, 3, 3]
    assert steps.cpu().numpy()[0, :10].tolist() == [0, 0, 0, 0, 1, 1, 0, 2, 2, GARBAGE]


def test_wrapper_returns_views_chunks_and_checks_on_the_host(dev, monkeypatch):
    _, ops = _mods()
    rng = np.random.default_rng(29)
    hyp, ref = E.random_rows(rng, [40] * 12, 40, ld=44), E.random_rows(rng, [33] * 4, 33, ld=35)
    hl, rl = rng.integers(0, 41, 12).astype(np.int32), rng.integers(0, 34, 4).astype(np.int32)
    want = A.reference(hyp, ref, hl, rl, R=3, hyp_cols=40, ref_cols=33)
    h, r = dv(hyp, dev)[:, :40], dv(ref, dev)[:, :33]

    def check(res):
        out, steps, ns = res
        assert out.shape == (12, 6) and steps.shape == (12, 73, 3) and ns.shape == (12,)
        assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(ns.cpu().numpy(), want[2])
        s = steps.cpu().numpy()
        assert all([tuple(t) for t in s[i, :want[2][i]].tolist()] == want[1][i] for i in range(12))

    check(ops.edit_align(h, r, dv(hl, dev), dv(rl, dev), R=3))
    check(ops.edit_align(h, r, dv(hl, dev), dv(rl, dev), R=3,
                         workspace=torch.full((ops.edit_align_workspace_elems(12, 40, 33),), -1, dtype=I32, device=dev)))
    # a cap that holds 7 pairs: pieces of 6 = two references' hypotheses, the same result
    monkeypatch.setattr(ops, "EDIT_ALIGN_WORKSPACE_CAP", 7 * 4 * ops.edit_align_workspace_elems(1, 40, 33))
    pieces = ops.edit_align_chunks(12, 3, 4 * ops.edit_align_workspace_elems(1, 40, 33), ops.EDIT_ALIGN_WORKSPACE_CAP)
    assert pieces == [(0, 6), (6, 6)]
    check(ops.edit_align(h, r, dv(hl, dev), dv(rl, dev), R=3))
    for args, kw in (((h.long(), r), dict(R=3)), ((h.cpu(), r), dict(R=3)), ((h, r), dict(R=2)), ((h[:, ::2], r), dict(R=3)),
                     ((h, r), dict(R=3, hyp_len=torch.zeros(5, dtype=I32, device=dev))),
                     ((h, r), dict(R=3, workspace=torch.zeros(8, dtype=I32, device=dev)))):
        with pytest.raises((ValueError, TypeError)):
            ops.edit_align(*args, **kw)


# ------------------------------------------------------------------------------------------------- tmi_edit_confusion
@pytest.fixture(scope="module")
def ctc_case(dev):
    """The CTC shape: 6 hypotheses of up to 300 tokens against 2 references of up to 200 (R = 3), tokens below V = 32 except
    one token equal to V and one negative token on each side."""
    _, ops = _mods()
    rng = np.random.default_rng(31)
    V, R = 32, 3
    hyp = rng.integers(0, V, (6, 300)).astype(np.int32)
    ref = rng.integers(0, V, (2, 200)).astype(np.int32)
    for b in range(2):  # the hypotheses are noisy copies of their reference, so matches dominate as in a real table
        for k in range(R):
            n = 200 - 10 * k
            hyp[3 * b + k, :n] = np.where(rng.random(n) < 0.8, ref[b, :n], hyp[3 * b + k, :n])
    hyp[0, 5], hyp[3, 17], ref[0, 9], ref[1, 40] = V, -4, -1, V
    hl = np.asarray([200, 190, 180, 300, 0, 120], np.int32)
    rl = np.asarray([200, 150], np.int32)
    h, r = dv(hyp, dev), dv(ref, dev)
    out, steps, ns = ops.edit_align(h, r, dv(hl, dev), dv(rl, dev), R=R)
    want = A.reference(hyp, ref, hl, rl, R=R)
    assert np.array_equal(ns.cpu().numpy(), want[2])
    return dict(V=V, R=R, hyp=hyp, ref=ref, hl=hl, rl=rl, h=h, r=r, steps=steps, ns=ns, want=want)


@pytest.mark.parametrize("first_only", [True, False])
def test_confusion_against_the_reference(dev, ctc_case, first_only):
    _, ops = _mods()
    c, V, R = ctc_case, ctc_case["V"], ctc_case["R"]
    got = ops.edit_confusion(c["steps"], c["ns"], c["h"], c["r"], V, R=R, first_only=first_only).cpu().numpy()
    want = A.confusion(c["want"][1], c["hyp"], c["ref"], V, R=R, first_only=first_only)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    pairs = [i for i in range(6) if not first_only or i % R == 0]
    assert got.sum() == sum(int(c["want"][2][i]) for i in pairs)  # the table and the trailing counter hold every counted step
    # the planted tokens, V and a negative one on each side, are counted in the trailing element (two of them could share a
    # substitution step, hence >= 2) and never indexed
    assert got[-1] == want[-1] and got[-1] >= 2
    # row sums without row V (insertions) = the histogram of the reference tokens in [0, V) of the counted pairs
    table = got[:-1].reshape(V + 1, V + 1)
    hist = np.zeros(V, np.int64)
    bad_ref = 0
    for i in pairs:
        toks = c["ref"][i // R][:c["rl"][i // R]]
        hist += np.bincount(toks[(toks >= 0) & (toks < V)], minlength=V)
        bad_ref += int(((toks < 0) | (toks >= V)).sum())
    # a reference token in [0, V) whose partner is outside [0, V) went to the trailing counter instead of its row
    moved = sum(1 for i in pairs for op, a, b in c["want"][1][i]
                if op in (A.MATCH, A.SUB) and 0 <= c["ref"][i // R][b] < V and not 0 <= c["hyp"][i][a] < V)
    assert (table[:V].sum(1) <= hist).all() and table[:V].sum() == hist.sum() - moved


def test_confusion_accumulates_over_batches(dev, ctc_case):
    _, ops = _mods()
    c, V, R = ctc_case, ctc_case["V"], ctc_case["R"]
    whole = ops.edit_confusion(c["steps"], c["ns"], c["h"], c["r"], V, R=R, first_only=False)
    counts = ops.edit_confusion(c["steps"][:3], c["ns"][:3], c["h"][:3], c["r"][:1], V, R=R, first_only=False)
    first = counts.clone()
    ret = ops.edit_confusion(c["steps"][3:], c["ns"][3:], c["h"][3:], c["r"][1:], V, R=R, first_only=False, counts=counts)
    assert ret.data_ptr() == counts.data_ptr()
    assert torch.equal(counts, whole) and not torch.equal(first, whole)
    again = ops.edit_confusion(c["steps"], c["ns"], c["h"], c["r"], V, R=R, first_only=False)
    assert torch.equal(again, whole)  # the same call, the same bits


def test_confusion_refusals_and_garbage_steps(dev, ctc_case):
    L, ops = _mods()
    lib, c, V = L.lib(), ctc_case, ctc_case["V"]
    counts = torch.full(((V + 1) ** 2 + 1 + 8,), GARBAGE, dtype=I32, device=dev)
    st, ns, h, r = c["steps"], c["ns"], c["h"], c["r"]
    good = dict(steps=st.data_ptr(), steps_ld=st.stride(0), n_steps=ns.data_ptr(), hyp=h.data_ptr(), hyp_ld=300, hyp_cols=300,
                ref=r.data_ptr(), ref_ld=200, ref_cols=200, N=6, R=3, first=1, V=V, counts=counts.data_ptr(), acc=0)

    def call(**over):
        a = dict(good, **over)
        return lib.tmi_edit_confusion(a["steps"], a["steps_ld"], a["n_steps"], a["hyp"], a["hyp_ld"], a["hyp_cols"], a["ref"],
                                      a["ref_ld"], a["ref_cols"], a["N"], a["R"], a["first"], a["V"], a["counts"], a["acc"], stream())

    for over in (dict(steps=None), dict(n_steps=None), dict(hyp=None), dict(ref=None), dict(counts=None), dict(V=0), dict(V=1025),
                 dict(first=2), dict(acc=-1), dict(N=0), dict(R=4), dict(steps_ld=1499), dict(hyp_ld=299), dict(ref_cols=4097),
                 dict(counts=counts.data_ptr() + 2), dict(steps=st.data_ptr() + 1)):
        assert call(**over) == TMI_ERR_INVALID, over
        assert lib.tmi_last_error()
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == GARBAGE).all()
    # steps that tmi_edit_align cannot have written (sentinel ops and columns, a length above the rows) are counted in the
    # trailing element and index nothing; the guard band behind counts stays
    junk = torch.full((6, 500, 3), GARBAGE, dtype=I32, device=dev)
    junk_n = torch.tensor([500, 7, -2, 9999, 0, 1], dtype=I32, device=dev)
    assert call(steps=junk.data_ptr(), steps_ld=1500, n_steps=junk_n.data_ptr(), first=0) == 0
    torch.cuda.synchronize()
    got = counts.cpu().numpy()
    assert (got[:(V + 1) ** 2] == 0).all() and got[(V + 1) ** 2] == 500 + 7 + 0 + 500 + 0 + 1 and (got[(V + 1) ** 2 + 1:] == GARBAGE).all()
