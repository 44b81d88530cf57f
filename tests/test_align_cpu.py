"""Host-side checks of the token-timestamp path: the new entry points in the header, the binding and the library; the
argument validator of ``align``; and tests/_align_ref.py itself - its median against scipy, its DTW against a plain double
loop and a brute force over all paths, the tie rule, an fp32 restatement of each kernel inside every bound, and the listed
mutations outside one.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _align_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tmi_align_cost", "tmi_align_cost_tile", "tmi_dtw", "tmi_dtw_workspace_bytes")
TINY = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, vocab_size=131, encoder_layers=2,
            decoder_layers=2, n_mels=8, n_ctx=96, decoder_start_token_id=130, max_target_positions=16)


def _lib():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib
    return _lib


# ----------------------------------------------------------------------------- the entry points
def test_entry_points_are_declared_bound_and_exported():
    L = _lib()
    header = open(os.path.join(ROOT, "include", "tethys_mi.h")).read()
    for name in NEW:
        m = re.search(r"(int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/tethys_mi.h"
        assert name in L.SIGNATURES
        assert len(L.SIGNATURES[name][1]) == len(m.group(2).split(",")), name
        assert hasattr(L.lib(), name)
    assert L.ABI_VERSION == 31 and L.lib().tmi_abi_version() == 31


def test_null_arguments_are_rejected_without_a_gpu():
    h = _lib().lib()
    assert h.tmi_align_cost(None, 0, 0, 0, None, None, None, None, 0, 0, 0, 0, 0, 0, 7, 1, 0, None) == -1
    assert b"tmi_align_cost" in h.tmi_last_error()
    assert h.tmi_dtw(None, 0, 0, None, None, 0, 0, 0, None, None, None, None, None, None, 0, None) == -1
    err = h.tmi_last_error()
    assert b"tmi_dtw" in err and b"1024" in err and b"4096" in err  # the limits that are built in
    assert h.tmi_dtw_workspace_bytes(1, 448, 1500) == 448 * 94 * 4
    assert h.tmi_dtw_workspace_bytes(1, 1025, 1500) == -1 and h.tmi_dtw_workspace_bytes(1, 448, 4097) == -1
    assert h.tmi_dtw_workspace_bytes(0, 448, 1500) == -1
    assert [h.tmi_align_cost_tile(w) for w in (1, 3, 5, 7, 9)] == [64, 62, 60, 58, 56]
    assert h.tmi_align_cost_tile(2) == -1 and h.tmi_align_cost_tile(11) == -1 and h.tmi_align_cost_tile(0) == -1


def test_check_align_args():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import whisper
    cfg = whisper.make_config("small", **TINY)
    chk = whisper.check_align_args
    a = chk(cfg, (4, 10), [3, 9, 9, 1], None, None, 7)
    assert (a["N"], a["n"], a["lengths"], a["num_frames"], a["medfilt_width"]) == (4, 9, [3, 9, 9, 1], None, 7)
    assert a["heads"] == [(1, 0), (1, 1)] and a["head_weights"] == {1: [0.5, 0.5]}  # the upper half of two layers
    a = chk(cfg, (2, 5), None, [96, 4], [(1, 1), (0, 0), (0, 1)], 1)
    assert a["lengths"] == [4, 4] and a["num_frames"] == [96, 4]
    third = 1.0 / 3.0
    assert a["heads"] == [(0, 0), (0, 1), (1, 1)] and a["head_weights"] == {0: [third, third], 1: [0.0, third]}
    assert chk(cfg, (1, 16), [15], None, [(0, 1)], 9)["head_weights"] == {0: [0.0, 1.0]}
    assert chk(cfg, (1, 1), None, None, None, 7)["n"] == 0
    assert abs(whisper.FRAME_SECONDS - 0.02) < 1e-15
    bad = [dict(seq_shape=(0, 5)), dict(seq_shape=(2,)), dict(seq_shape=(2, 0)),
           dict(lengths=[1, 2, 3]), dict(lengths=[5, 1]), dict(lengths=[-1, 1]),
           dict(seq_shape=(2, 17)),                      # 1 + 16 tokens: no decoder position for the last one
           dict(num_frames=[3, 50]), dict(num_frames=[97, 50]), dict(num_frames=[]),
           dict(alignment_heads=[(0, 0), (0, 0)]), dict(alignment_heads=[(2, 0)]), dict(alignment_heads=[(0, 2)]),
           dict(alignment_heads=[(-1, 0)]), dict(alignment_heads=[]), dict(alignment_heads=[3]), dict(alignment_heads=5),
           dict(medfilt_width=0), dict(medfilt_width=2), dict(medfilt_width=11), dict(medfilt_width=3.5),
           dict(medfilt_width=True)]
    for kw in bad:
        args = dict(seq_shape=(2, 5), lengths=None, num_frames=None, alignment_heads=None, medfilt_width=7)
        args.update(kw)
        with pytest.raises(ValueError):
            chk(cfg, **args)
    with pytest.raises(ValueError):
        whisper.check_timestamp_length(cfg, 16)
    assert whisper.check_timestamp_length(cfg, None) == 15 and whisper.check_timestamp_length(cfg, 3) == 3


def test_transcribe_cli_has_the_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "speech_jobs", "whisper_transcribe.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--timestamps" in r.stdout


# ----------------------------------------------------------------------------- the reference: median
@pytest.mark.parametrize("width", [1, 3, 5, 7, 9])
def test_median_equals_scipy_mirror(width):
    from scipy.ndimage import median_filter
    z = np.random.default_rng(width).standard_normal((5, 41))
    for cols in (width // 2 + 1, 7, 41):
        got = A.median_ref(z[:, :cols], width)
        ref = median_filter(z[:, :cols], size=(1, width), mode="mirror")
        assert np.array_equal(got, ref), (width, cols)
    pad = np.pad(z, ((0, 0), (width // 2, width // 2)), mode="reflect")
    win = np.stack([pad[:, k:k + 41] for k in range(width)], axis=-1)
    assert np.array_equal(A.median_ref(z, width), np.median(win, axis=-1))


# ----------------------------------------------------------------------------- the reference: DTW
def test_dtw_equals_the_plain_loop():
    for R, Cn, seed in ((1, 1, 0), (1, 7, 1), (5, 1, 2), (2, 2, 3), (9, 13, 4), (13, 9, 5), (20, 33, 6)):
        for c in (A.grid_cost(R, Cn, seed), A.random_cost(R, Cn, seed), np.round(A.grid_cost(R, Cn, seed) / 8)):  # (the last: many ties)
            D, mv = A.dtw_tables(c)
            Dp, mvp = A.dtw_plain(c)
            assert np.array_equal(D, Dp) and np.array_equal(mv, mvp)
            r = A.dtw_ref(c)
            assert A.path_problems(r["path"], R, Cn, r["start"], r["end"]) == []
            assert r["total"] == D[-1, -1]


def test_dtw_equals_brute_force_4x5():
    paths = [np.asarray(p) for p in A.all_paths(4, 5)]
    assert len(paths) == 129  # the Delannoy number D(3, 4)
    for seed in range(20):
        c = A.random_cost(4, 5, seed) if seed % 2 else A.grid_cost(4, 5, seed)
        costs = np.array([A.path_cost(c, p) for p in paths])
        r = A.dtw_ref(c)
        assert abs(r["total"] - costs.min()) <= 1e-12
        if (np.abs(costs - costs.min()) <= 1e-12).sum() == 1:  # a unique optimum: the traced path is that path
            assert np.array_equal(r["path"], paths[int(costs.argmin())])
            assert abs(A.path_cost(c, r["path"]) - r["total"]) <= 1e-12


def test_tie_rule_on_an_all_zero_cost():
    """Every comparison ties, so every interior move is "left", the first column moves up: traced back from the last cell
    the path runs left along the last row and then up the first column."""
    r = A.dtw_ref(np.zeros((4, 6)))
    want = [(i, 0) for i in range(4)] + [(3, j) for j in range(1, 6)]
    assert [tuple(x) for x in r["path"]] == want
    assert list(r["start"]) == [0, 0, 0, 0] and list(r["end"]) == [1, 1, 1, 6] and r["total"] == 0.0
    assert [tuple(x) for x in A.dtw_ref(np.zeros((4, 6)), variant="tie_diag")["path"]] != want  # the mutation shows


def test_grid_costs_are_exact_in_fp32():
    c = A.grid_cost(40, 65, 3)
    a, b = A.dtw_ref(c, np.float32), A.dtw_ref(c, np.float64)
    assert np.array_equal(a["path"], b["path"]) and float(a["total"]) == float(b["total"])


# ----------------------------------------------------------------------------- the bounds: honest fp32 inside, mutations outside
def _cost_case(dtype, width, normalize, seed=11):
    rows, cols = [17, 2, 1], [131, 59, 5]
    p = A.cost_inputs(3, 3, 17, 131, dtype, seed)
    hw = np.array([0.5, 0.0, 0.5], dtype=np.float32)
    return p, rows, cols, hw


@pytest.mark.parametrize("dtype", [A.F32, A.BF16])
@pytest.mark.parametrize("width", [1, 3, 7, 9])
@pytest.mark.parametrize("normalize", [True, False])
def test_fp32_cost_restatement_is_inside_the_bound(dtype, width, normalize):
    p, rows, cols, hw = _cost_case(dtype, width, normalize)
    ref, bound = A.cost_ref(p, rows, cols, hw, width, normalize)
    got = A.cost_f32(p, rows, cols, hw, width, normalize)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert A.ratio(torch.from_numpy(got[ok]), torch.from_numpy(ref[ok]), torch.from_numpy(bound[ok])) <= 1.0
    if normalize:
        assert np.all(got[2, :1, :5] == 0) and np.all(ref[2, :1, :5] == 0)  # one token: exactly zero
        # the bound is tight enough to mean something: a few hundred roundings of values of order 1
        assert np.nanmax(bound[0]) < 1e-4
    else:
        assert np.nanmax(bound) <= A.gam(2) * np.nanmax(np.abs(ref)) * 1.01
    # accumulate: onto the first result
    ref2, bound2 = A.cost_ref(p[:, ::-1], rows, cols, hw, width, normalize, base=got)
    got2 = A.cost_f32(p[:, ::-1], rows, cols, hw, width, normalize, base=got)
    assert A.ratio(torch.from_numpy(got2[ok]), torch.from_numpy(ref2[ok]), torch.from_numpy(bound2[ok])) <= 1.0


def test_one_head_of_weight_one_without_normalisation_is_exact():
    p = A.cost_inputs(1, 1, 9, 70, A.BF16, 5)
    ref, bound = A.cost_ref(p, [9], [70], np.ones(1, np.float32), 7, False)
    got = A.cost_f32(p, [9], [70], np.ones(1, np.float32), 7, False)
    assert np.array_equal(got.astype(np.float64), ref)
    assert np.array_equal(ref[0], -A.median_ref(p[0, 0], 7))


@pytest.mark.parametrize("variant", ["sample_var", "edge"])
def test_cost_mutations_exceed_the_bound(variant):
    p, rows, cols, hw = _cost_case(A.F32, 7, True)
    ref, bound = A.cost_ref(p, rows, cols, hw, 7, True)
    got = A.cost_f32(p, rows, cols, hw, 7, True, variant=variant)
    ok = ~np.isnan(ref) & np.isfinite(bound) & ~np.isnan(got)
    assert A.ratio(torch.from_numpy(got[ok]), torch.from_numpy(ref[ok]), torch.from_numpy(bound[ok])) > 1.0


@pytest.mark.parametrize("shape", [(65, 300), (448, 1500)])
def test_fp32_dtw_restatement_is_inside_the_bound(shape):
    c = A.random_cost(*shape, seed=shape[0])
    ref = A.dtw_ref(c)
    got = A.dtw_ref(c, np.float32)
    assert A.path_problems(got["path"], *shape, got["start"], got["end"]) == []
    excess_bound, total_bound = A.dtw_bounds(c, ref, got["path"])
    assert 0.0 <= A.path_cost(c, got["path"]) - ref["total"] <= excess_bound
    assert abs(float(got["total"]) - ref["total"]) <= total_bound
    assert excess_bound < 1e-3 * abs(ref["total"])  # (a bound that means something)


@pytest.mark.parametrize("variant", ["tie_diag", "no_up"])
def test_dtw_mutations_break_a_check(variant):
    if variant == "tie_diag":  # exact cases: ties are part of the answer
        c = np.round(A.grid_cost(20, 33, 6) / 8)
        assert not np.array_equal(A.dtw_ref(c, variant=variant)["path"], A.dtw_ref(c)["path"])
    else:  # a dropped predecessor: no longer the optimum
        c = A.random_cost(65, 300, seed=65)
        ref, got = A.dtw_ref(c), A.dtw_ref(c, np.float32, variant=variant)
        excess_bound, total_bound = A.dtw_bounds(c, ref, got["path"])
        assert A.path_cost(c, got["path"]) - ref["total"] > excess_bound or abs(float(got["total"]) - ref["total"]) > total_bound
