"""The GEMM checker checked on the CPU (no GPU needed): for every case of the form table (tests/_gemm_forms.py) the
descriptor-level reference must equal an independent formulation of the same call to float64 round-off, and its
per-element bound must SEE each of a list of wrong results a subtly broken kernel could produce - a bound that cannot is a
test that cannot fail."""
import numpy as np
import pytest

import _gemm_forms as F
import _gemm_ref as R

NAMES = [c["name"] for c in F.CASES]


@pytest.fixture(scope="module", params=NAMES)
def prepared(request):
    """(name, buffers, references) of one case: module-scoped, so both tests of a case run on one preparation."""
    return (request.param,) + F.prepare(F.BY_NAME[request.param])


def test_reference_equals_independent_formulation(prepared):
    name, bufs, refs = prepared
    case = F.BY_NAME[name]
    outs = case["indep"](bufs)
    assert len(outs) == len(refs)
    for L, r, (o, aux) in zip(case["launches"], refs, outs):
        assert np.isfinite(r["ref"]).all() and np.isfinite(r["bound"]).all() and (r["bound"] > 0).all()
        o = np.asarray(o).reshape(r["ref"].shape)
        # float64 round-off of two summation orders of K_total terms: K_total * 2^-53 * sum |a||b| is far below this
        scale = np.abs(r["ref"]).max()
        assert np.abs(o - r["ref"]).max() <= 1e-12 * scale, name
        if L.get("aux_out"):
            assert aux is not None
            assert np.abs(np.asarray(aux).reshape(r["ref"].shape) - r["aux_ref"]).max() <= 1e-12 * np.abs(r["aux_ref"]).max()
        # the window is what the call may write, nothing else
        assert r["written"].size == r["ref"].size


def test_case_names_and_expectations_are_complete():
    for c in F.CASES:
        assert c["expect"] is not None and len(c["expect"]) == 3, c["name"]
        assert c["site"], c["name"]


# ------------------------------------------------------------------------------------------------ wrong results
def _violates(got, ref, bound):
    return R.worst_ratio(got, ref, bound) > 1.0


def _tile(r, m0=0, n0=0):
    M, N = r["ref"].shape[2:]
    return slice(m0, min(M, m0 + 64)), slice(n0, min(N, n0 + 64))


def _ktile_delta(r, sign):
    """One 64-wide K-tile (the first) of one 64 x 64 output tile (the first), missing (sign -1) or added twice (+1)."""
    ms, ns = _tile(r)
    a, b = r["a_g"][0, 0, ms, :64], r["b_g"][0, 0, ns, :64]
    d = np.zeros_like(r["ref"])
    d[0, 0, ms, ns] = sign * (a @ b.T)
    return d


MUTATIONS = ("ktile_missing", "ktile_twice", "element_stale", "rows_swapped", "scale_one_column_more", "bias_missing_last_chunk",
             "gelu_on_aux_out", "resid_read_with_ldc")


def _mutate(case, L, bufs, r, what):
    """-> (got, ref, bound) of the wrong result `what`, or None where the launch has no such feature."""
    rnd = lambda x: F.round_to(x, case["out_bf16"])
    good = rnd(r["ref"])
    if what in ("ktile_missing", "ktile_twice"):
        wrong = F.ref_launch(case, L, bufs, M=L["M"], acc_delta=_ktile_delta(r, -1.0 if what == "ktile_missing" else 1.0))
        return rnd(wrong["ref"]), r["ref"], r["bound"]
    if what == "element_stale":
        got = good.copy()
        # the element whose new value is furthest from its old one, measured in bounds (NaN beforehand: any element)
        old = bufs["C"][r["c_idx"]]
        score = np.where(np.isnan(old), np.inf, np.abs(old - r["ref"]) / r["bound"])
        i = np.unravel_index(np.argmax(score), score.shape)
        got[i] = old[i]
        return got, r["ref"], r["bound"]
    if what == "rows_swapped":
        got = good.copy()
        got[0, 0, [4, 5]] = got[0, 0, [5, 4]]
        return got, r["ref"], r["bound"]
    if what == "scale_one_column_more":
        sc = L.get("scale_cols", 0)
        if not 0 < sc < L["N"]:
            return None
        wrong = F.ref_launch(case, L, bufs, M=L["M"], scale_cols=sc + 1)
        return rnd(wrong["ref"]), r["ref"], r["bound"]
    if what == "bias_missing_last_chunk":
        if not L.get("bias"):
            return None
        bo, N = L.get("bias_off", 0), L["N"]
        bias = bufs["bias"][bo:].copy()
        for b in range(max(1, L.get("nbatch", 1))):
            bias[b * L.get("bias_sb", 0) + 8 * ((N - 1) // 8):b * L.get("bias_sb", 0) + N] = 0.0
        wrong = F.ref_launch(case, L, bufs, M=L["M"], bias=bias)
        return rnd(wrong["ref"]), r["ref"], r["bound"]
    if what == "gelu_on_aux_out":
        if not L.get("aux_out"):
            return None
        return rnd(R.gelu(r["aux_ref"])), r["aux_ref"], r["aux_bound"]
    if what == "resid_read_with_ldc":
        if not L.get("resid") or L["r_ld"] == L["ldc"]:
            return None
        resid = np.concatenate([bufs["resid"], np.full(L["M"] * L["ldc"] * max(1, L.get("nbatch", 1)), np.nan)])
        wrong = F.ref_launch(case, L, bufs, M=L["M"], resid=resid, r_ld=L["ldc"])
        return rnd(wrong["ref"]), r["ref"], r["bound"]
    raise AssertionError(what)


def test_bound_sees_every_wrong_result(prepared):
    """Every wrong result is built in the first 128 rows of the window (where the launch has more, the rows below are left
    correct, which takes nothing from the check: one violated element is what has to be shown)."""
    name, bufs, refs = prepared
    case = F.BY_NAME[name]
    for L, r in zip(case["launches"], refs):
        # the correctly rounded reference itself is within the bound, everywhere
        assert R.worst_ratio(F.round_to(r["ref"], case["out_bf16"]), r["ref"], r["bound"]) <= 1.0
        if L["M"] > 128:
            L = dict(L, M=128)
            r = dict(r, **{k: r[k][:, :, :128] for k in ("ref", "bound", "c_idx", "a_g", "aux_ref", "aux_bound") if k in r})
        for what in MUTATIONS:
            m = _mutate(case, L, bufs, r, what)
            if m is not None:
                assert _violates(*m), (name, what)


def test_every_wrong_result_is_exercised_by_some_case():
    seen = set()
    for c in F.CASES:
        for L in c["launches"]:
            seen.add("ktile_missing"), seen.add("ktile_twice"), seen.add("element_stale"), seen.add("rows_swapped")
            if 0 < L.get("scale_cols", 0) < L["N"]:
                seen.add("scale_one_column_more")
            if L.get("bias"):
                seen.add("bias_missing_last_chunk")
            if L.get("aux_out"):
                seen.add("gelu_on_aux_out")
            if L.get("resid") and L["r_ld"] != L["ldc"]:
                seen.add("resid_read_with_ldc")
    assert seen == set(MUTATIONS)


def test_can_run_matches_the_forced_kernel_conditions():
    """A few fixed points of F.can_run (the conditions at the top of launch_fast)."""
    lin = F.BY_NAME["linear_bias"]["launches"][0]
    assert all(F.can_run(lin, False, cfg) for cfg in F.FORCED)
    wg = F.BY_NAME["wgrad_nosplit"]["launches"][0]           # K = 200: a K tail, both operands k-strided
    assert [cfg for cfg in F.FORCED if F.can_run(wg, False, cfg)] == [4, 5, 6, 12, 13, 10]
    qd = F.BY_NAME["w2v_qkv_dgrad"]["launches"][0]           # kbatch = 3: not the eight-phase kernel
    assert not F.can_run(qd, False, 10) and not F.can_run(qd, False, 14) and F.can_run(qd, False, 15)
    assert not any(F.can_run(F.BY_NAME["parity_scores"]["launches"][0], True, cfg) for cfg in F.FORCED)
    assert not any(F.can_run(F.BY_NAME["contrastive_dph_generic"]["launches"][0], False, cfg) for cfg in F.FORCED)
