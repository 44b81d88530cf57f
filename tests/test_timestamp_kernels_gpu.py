"""tmi_timestamp_rules and tmi_lm_head_timestamp_gate on the GPU against tests/_timestamp_ref.py.  Inputs and expected
results are built on the host by the reference; tests/test_timestamp_cpu.py shows from the reference alone that the
planted rule g inputs have no undecided row and the random tier at most 5 %."""
import itertools

import numpy as np
import pytest
import torch

import _constrain_ref as C
import _timestamp_ref as T

pytestmark = pytest.mark.gpu

GARBAGE = 0x7BADBEEF


def _mods():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops
    return ops, _lib


def _bits(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ----------------------------------------------------------------------------- 1. rules a - f, bit for bit
@pytest.mark.parametrize("V,tb", T.RULE_SHAPES)
def test_timestamp_rules_equal_reference(dev, V, tb):
    """M in {1, 5, 17} x P in {0, 3} x the states of _timestamp_ref.rule_case (n = 0, 1, 2 and longer; opening, closing,
    pair, text; tl at tb + max_ts; ids -1, V and 2^31 - 1 in the row; timestamps past t that would change the state),
    on top of a caller's random bans: every word equals the reference's, the sentinel word past W survives, and two calls
    give equal bits (the second one on the first one's output: the rules only add, so nothing may change)."""
    ops, _ = _mods()
    n = 0
    for M, P in itertools.product(T.RULE_MS, T.RULE_PS):
        for c in T.rule_case(M, V, tb, P):
            prefix = torch.from_numpy(c["prefix"]).to(dev)
            banned = _bits(c["banned"], dev)
            kw = dict(no_timestamps_id=c["no_ts"], eos_id=c["eos"], max_initial=c["max_initial"], max_ts=c["max_ts"])
            ops.timestamp_rules(prefix, c["ld"], M, c["t"], P, V, tb, banned, **kw)
            got = _u32(banned)
            exp = T.rule_expected(c)
            bad = np.nonzero((got != exp).any(axis=1))[0]
            assert not len(bad), (M, V, P, c["t"], [c["names"][r] for r in bad])
            ops.timestamp_rules(prefix, c["ld"], M, c["t"], P, V, tb, banned, **kw)
            assert np.array_equal(_u32(banned), got), ("a second call changed bits", M, V, P, c["t"])
            fresh = _bits(c["banned"], dev)
            ops.timestamp_rules(prefix, c["ld"], M, c["t"], P, V, tb, fresh, **kw)
            assert np.array_equal(_u32(fresh), got), ("two calls differ", M, V, P, c["t"])
            n += 1
    assert n == len(T.RULE_MS) * len(T.RULE_PS) * 4


def test_timestamp_rules_refusals(dev):
    ops, _lib = _mods()
    h = _lib.lib()
    V, tb, M, t, ld, P = 200, 137, 3, 5, 8, 1
    W = C.words(V)
    prefix = torch.zeros(M, ld, dtype=torch.int32, device=dev)
    banned = torch.full((M, W), GARBAGE, dtype=torch.int32, device=dev)
    ok = dict(prefix=prefix.data_ptr(), ld=ld, M=M, t=t, P=P, V=V, tb=tb, no_ts=tb - 1, eos=2, mi=5, mt=50,
              banned=banned.data_ptr(), bits_ld=W)
    bad = [dict(prefix=None), dict(banned=None), dict(banned=banned.data_ptr() + 2), dict(M=0), dict(M=65536), dict(V=0),
           dict(V=65537), dict(t=0), dict(t=ld + 1), dict(t=65537, ld=70000), dict(P=-1), dict(P=t), dict(tb=-1), dict(tb=V + 1),
           dict(no_ts=V), dict(eos=V), dict(mt=-1), dict(bits_ld=W - 1)]
    for change in bad:
        a = dict(ok, **change)
        rc = h.tmi_timestamp_rules(a["prefix"], a["ld"], a["M"], a["t"], a["P"], a["V"], a["tb"], a["no_ts"], a["eos"],
                                   a["mi"], a["mt"], a["banned"], a["bits_ld"], ops.stream())
        assert rc == -1, (change, rc)  # TMI_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((banned == GARBAGE).all()), "a refused call wrote its output"
    # the limits themselves pass: V = 65536 with tb = V (no timestamp id at all) and a prefix of 2^16 tokens
    Vb = 65536
    big = torch.full((1, 65536), 7, dtype=torch.int32, device=dev)
    b2 = torch.zeros(1, C.words(Vb), dtype=torch.int32, device=dev)
    ops.timestamp_rules(big, 65536, 1, 65536, 0, Vb, Vb, b2, no_timestamps_id=-1, eos_id=-1, max_initial=-1, max_ts=1 << 40)
    assert not _u32(b2).any()
    ops.timestamp_rules(big, 65536, 1, 1, 0, Vb, Vb, b2, no_timestamps_id=9, eos_id=-1, max_initial=-1, max_ts=0)
    assert np.array_equal(_u32(b2)[0], C.bitset(range(Vb), Vb))  # (n = 0: every below column)


# ----------------------------------------------------------------------------- 2. rule g
def _gate(ops, x, x_ld, w, w_ld, M, d, V, tb, seen, banned, penalty, ws=None, gamma=None, beta=None):
    dev = w.device
    fired = torch.full((M,), -7, dtype=torch.int32, device=dev)
    fresh = ws is None
    ws = torch.zeros(ops.lm_head_timestamp_gate_workspace_elems(M, V), dtype=torch.int64, device=dev) if fresh else ws
    ops.lm_head_timestamp_gate(x, x_ld, w, w_ld, M, d, V, tb, fired, ws, seen=seen, banned=banned, penalty=penalty,
                               gamma=gamma, beta=beta)
    if fresh:
        torch.cuda.synchronize()
        assert int(ws.abs().sum()) == 0, "the workspace is not left zero"
    return fired.cpu().numpy()


def _check_gate(name, fired, seen_d, banned_d, ref_fired, decided, seen0, banned0, tb, V, W):
    assert set(np.unique(fired)) <= {0, 1}, (name, fired)
    bad = np.nonzero(decided & (fired.astype(bool) != ref_fired))[0]
    assert not len(bad), (name, "decided rows differ", bad, fired[bad], ref_fired[bad])
    assert np.array_equal(_u32(seen_d), seen0), (name, "seen was written")
    # only below bits are added, and only on the rows that fired (by the kernel's own account); everything else, the bits at
    # or above V and the sentinel word included, is as it was
    assert np.array_equal(_u32(banned_d), T.gate_banned(banned0, fired, tb, V)), (name, "banned")


@pytest.mark.parametrize("wdt", ("bf16", "fp32"))
@pytest.mark.parametrize("M", T.GATE_MS)
def test_gate_planted_rows(dev, wdt, M):
    """d = 64, V = 200 with tb = 137, the planted rows of _timestamp_ref.planted_case (fire / no fire, the spread row that
    only the LSE fires, every timestamp column banned, every below column banned, the row only the penalty fires, every
    column banned, random sets), bits at or above V set in both sets: every row is decided and must match; seen is
    untouched; only below bits are added, only on fired rows; the workspace is left zero; a second call on fresh copies
    gives the same bits."""
    ops, _ = _mods()
    V, tb = T.GATE_SMALL
    c = T.planted_case(M, V, tb)
    dt = torch.bfloat16 if wdt == "bf16" else torch.float32
    x, w = torch.from_numpy(c["x"]).to(dev).to(dt), torch.from_numpy(c["w"]).to(dev).to(dt)
    outs = []
    for _ in range(2):
        seen, banned = _bits(c["seen"], dev), _bits(c["banned"], dev)
        fired = _gate(ops, x, T.GATE_D, w, c["VP"], M, T.GATE_D, V, tb, seen, banned, T.GATE_PENALTY)
        _check_gate((wdt, M, c["names"]), fired, seen, banned, c["fired"], c["decided"], c["seen"], c["banned"], tb, V, c["W"])
        outs.append((fired, _u32(banned)))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert c["decided"].all()


def test_gate_full_vocabulary(dev):
    """V = 51865 with tb = 50364 (406 workgroups a row tile: the fold's strided part and its butterfly both run), M = 8,
    bf16: the planted rows again."""
    ops, _ = _mods()
    V, tb = T.GATE_LARGE
    M = 8
    c = T.planted_case(M, V, tb)
    x, w = torch.from_numpy(c["x"]).to(dev).bfloat16(), torch.from_numpy(c["w"]).to(dev).bfloat16()
    seen, banned = _bits(c["seen"], dev), _bits(c["banned"], dev)
    fired = _gate(ops, x, T.GATE_D, w, c["VP"], M, T.GATE_D, V, tb, seen, banned, T.GATE_PENALTY)
    _check_gate(("full", c["names"]), fired, seen, banned, c["fired"], c["decided"], c["seen"], c["banned"], tb, V, c["W"])


@pytest.mark.parametrize("case", T.RANDOM_CASES, ids=lambda c: f"{c[0]}-M{c[4]}")
def test_gate_random_rows_with_layernorm(dev, case):
    """Random activations through the LayerNorm, random sets, penalty 1.3, rows read at a stride (every third row of x),
    M = 40 (three row tiles, the last one partial): every decided row matches the fp64 reference."""
    ops, _ = _mods()
    wdt, d, V, tb, M, _seed = case
    c = T.random_case(*case)
    x, w = c["x"].to(dev), c["w"].to(dev)
    gamma, beta = c["gamma"].to(dev), c["beta"].to(dev)
    seen, banned = _bits(c["seen"], dev), _bits(c["banned"], dev)
    fired = _gate(ops, x[2:], 3 * d, w, c["VP"], M, d, V, tb, seen, banned, T.RANDOM_PENALTY, gamma=gamma, beta=beta)
    _check_gate(case, fired, seen, banned, c["fired"], c["decided"], c["seen"], c["banned"], tb, V, c["W"])


def test_gate_alternates_with_topk_c_on_one_workspace(dev):
    """The gate and tmi_lm_head_topk_c, turn by turn on one stream and ONE zeroed buffer sized for both: each leaves it
    zero, so each finds it zero; the gate's bans are what the top-k call then sees (a fired row's candidates are
    timestamps), and the results repeat."""
    ops, _ = _mods()
    V, tb = T.GATE_SMALL
    M, N, d = 17, 4, T.GATE_D
    c = T.planted_case(M, V, tb)
    x, w = torch.from_numpy(c["x"]).to(dev).bfloat16(), torch.from_numpy(c["w"]).to(dev).bfloat16()
    n_ws = max(ops.lm_head_timestamp_gate_workspace_elems(M, V), ops.lm_head_topk_workspace_elems(M, V, N))
    ws = torch.zeros(n_ws, dtype=torch.int64, device=dev)
    rounds = []
    for _ in range(3):
        seen, banned = _bits(c["seen"], dev), _bits(c["banned"], dev)
        fired = _gate(ops, x, d, w, c["VP"], M, d, V, tb, seen, banned, T.GATE_PENALTY, ws=ws)
        ids = torch.full((M, N), -7, dtype=torch.int32, device=dev)
        lp = torch.full((M, N), float("nan"), device=dev)
        ops.lm_head_topk_c(x, d, w, c["VP"], M, d, V, N, ids, lp, ws, seen=seen, banned=banned, penalty=T.GATE_PENALTY)
        rounds.append((fired, ids.cpu().numpy(), lp.cpu().numpy()))
    torch.cuda.synchronize()
    assert int(ws.abs().sum()) == 0, "the shared workspace is not left zero"
    for fired, ids, lp in rounds:
        assert np.array_equal(fired.astype(bool), c["fired"])
        assert np.array_equal(fired, rounds[0][0]) and np.array_equal(ids, rounds[0][1]) and np.array_equal(lp, rounds[0][2])
        for r in np.nonzero(fired)[0]:
            live = np.isfinite(lp[r])
            assert live.any() and (ids[r][live] >= tb).all(), (r, c["names"][r], ids[r], lp[r])


def test_gate_refusals(dev):
    ops, _lib = _mods()
    h = _lib.lib()
    V, tb, M, d = 200, 137, 3, 64
    W = C.words(V)
    x = torch.zeros(M, d, device=dev)
    w = torch.zeros(d, 200, device=dev)
    gamma = torch.ones(d, device=dev)
    seen = torch.zeros(M, W, dtype=torch.int32, device=dev)
    banned = torch.full((M, W), GARBAGE, dtype=torch.int32, device=dev)
    fired = torch.full((M,), -7, dtype=torch.int32, device=dev)
    nb = h.tmi_lm_head_timestamp_gate_workspace_bytes(M, V)
    assert nb == 16 * M * (1 + 2) and h.tmi_lm_head_timestamp_gate_workspace_bytes(0, V) == -1
    assert h.tmi_lm_head_timestamp_gate_workspace_bytes(M, 65537) == -1
    ws = torch.zeros(nb // 8 + 2, dtype=torch.int64, device=dev)
    ok = dict(x=x.data_ptr(), x_ld=d, xdt=0, gamma=None, beta=None, w=w.data_ptr(), w_ld=200, wdt=0, M=M, d=d, V=V,
              seen=seen.data_ptr(), banned=banned.data_ptr(), bits_ld=W, penalty=1.0, tb=tb, fired=fired.data_ptr(),
              ws=ws.data_ptr(), ws_bytes=nb)
    bad = [dict(x=None), dict(w=None), dict(banned=None), dict(fired=None), dict(ws=None), dict(ws=ws.data_ptr() + 8),
           dict(ws_bytes=nb - 1), dict(M=0), dict(V=0), dict(tb=-1), dict(tb=V + 1), dict(penalty=0.0),
           dict(penalty=float("inf")), dict(bits_ld=W - 1), dict(gamma=gamma.data_ptr()), dict(xdt=2), dict(w_ld=V - 8),
           dict(w_ld=204), dict(x_ld=d - 1), dict(banned=banned.data_ptr() + 2), dict(d=100000, x_ld=100000)]
    for change in bad:
        a = dict(ok, **change)
        rc = h.tmi_lm_head_timestamp_gate(a["x"], a["x_ld"], a["xdt"], a["gamma"], a["beta"], 1e-5, a["w"], a["w_ld"], a["wdt"],
                                          a["M"], a["d"], a["V"], a["seen"], a["banned"], a["bits_ld"], a["penalty"], a["tb"],
                                          a["fired"], a["ws"], a["ws_bytes"], ops.stream())
        assert rc == -1, (change, rc)  # TMI_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((banned == GARBAGE).all()) and bool((fired == -7).all()) and int(ws.abs().sum()) == 0
    # seen may be NULL; tb = V (no timestamp column) never fires, tb = 0 (no below column) fires on any live column
    banned.zero_()
    for tb2, want in ((V, 0), (0, 1)):
        rc = h.tmi_lm_head_timestamp_gate(ok["x"], d, 0, None, None, 1e-5, ok["w"], 200, 0, M, d, V, None, ok["banned"], W, 1.0,
                                          tb2, ok["fired"], ok["ws"], nb, ops.stream())
        assert rc == 0
        assert fired.cpu().tolist() == [want] * M and not _u32(banned).any()
