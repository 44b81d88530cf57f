"""tests/_layout_ref.py checked without a GPU: the bf16 conversion against torch's, the index maps against plain tensor
operations, the log-mel reference and its bound (an honest fp32 restatement of the kernel's loop stays inside, each listed
wrong implementation exceeds it by orders of magnitude), dropout_expected, and - for every rate, seed and shape the GPU files
use - that the oracle's mask has the intended threshold, the expected keep fraction, and at least one kept and one dropped
element, so that no GPU case passes while checking nothing."""
import math

import numpy as np
import pytest
import torch

import _layout_ref as L
import _row_kernel_ref as R
from oracle import dropout as DO

F32, BF16, F64 = L.F32, L.BF16, L.F64


# ================================================================================================= bf16
def test_bf16_full_is_torch_rounding_and_names_the_special_results():
    x = L.special_input((97, 53), 5, 3.0)
    got, want = L.bf16_full(x), x.to(BF16)
    ok = ~torch.isnan(x)
    assert torch.equal(L.bits(got)[ok], L.bits(want)[ok]) and bool(torch.isnan(got[~ok]).all())
    assert int((~ok).sum()) >= 3 * (x.numel() // 84 - 1)
    w = {word: int(L.bits(L.bf16_full(L.SPECIAL[i:i + 1]))[0]) & 0xFFFF for i, word in enumerate(L.SPECIAL_WORDS)}
    assert w[0x3F808000] == 0x3F80 and w[0x3F818000] == 0x3F82          # ties: to even, both ways
    assert w[0x3F807FFF] == 0x3F80 and w[0x3F808001] == 0x3F81 and w[0x3F817FFF] == 0x3F81 and w[0x3F818001] == 0x3F82
    assert w[0xBF808000] == 0xBF80 and w[0xBF818000] == 0xBF82
    assert w[0x00000000] == 0x0000 and w[0x80000000] == 0x8000
    assert w[0x7F7F0000] == 0x7F7F and w[0x7F7F7FFF] == 0x7F7F and w[0x7F7F8000] == 0x7F80 and w[0x7F7F8001] == 0x7F80
    assert w[0xFF7F8001] == 0xFF80 and w[0x7F800000] == 0x7F80 and w[0xFF800000] == 0xFF80
    assert w[0x00000001] == 0x0000 and w[0x007FFFFF] == 0x0080 and w[0x80000001] == 0x8000
    assert w[0x00008000] == 0x0000 and w[0x00018000] == 0x0002
    for word in (0x7FC00000, 0x7F800001, 0xFFFFFFFF):
        assert (w[word] & 0x7F80) == 0x7F80 and (w[word] & 0x7F) != 0
    assert float(torch.finfo(BF16).max) == (2.0 - 2.0 ** -7) * 2.0 ** 127
    assert L.BF16_OVERFLOW == (2.0 - 2.0 ** -8) * 2.0 ** 127               # half way from the largest bf16 to 2^128


def test_same_bits_tells_a_truncating_cast_and_a_wrong_zero():
    x = L.special_input((40, 21), 6)
    want = L.bf16_full(x)
    assert L.same_bits(want.clone(), want)
    trunc = (L.bits(x) >> 16).to(torch.int16).view(BF16)          # no rounding: sNaN 0x7F800001 becomes inf, ties go down
    assert not L.same_bits(trunc, want)
    flipped = want.clone()
    flipped.view(torch.int16)[x == 0] ^= -0x8000                   # +0 <-> -0
    assert not L.same_bits(flipped, want)
    anynan = want.clone()
    anynan.view(torch.int16)[torch.isnan(want)] = -1               # another NaN pattern is accepted
    assert L.same_bits(anynan, want)


# ================================================================================================= index maps
@pytest.mark.parametrize("rows,cols,lds,ldd,so,do", [(7, 5, 9, 8, 0, 0), (3, 4, 4, 4, 3, 5), (1, 1, 1, 1, 0, 0)])
def test_cast_and_transpose_are_their_index_maps(rows, cols, lds, ldd, so, do):
    src = L.special_input((so + rows * lds + 3,), 7)
    idx, val = L.cast_ref(src, rows, cols, lds, ldd, so, do)
    assert idx.numel() == rows * ldd == idx.unique().numel()
    for r in range(rows):
        for c in range(ldd):
            k = r * ldd + c
            assert int(idx[k]) == do + r * ldd + c
            want = L.bf16_full(src[so + r * lds + c].reshape(1)) if c < cols else torch.zeros(1, dtype=BF16)
            assert L.same_bits(val[k:k + 1], want)
    ldt = rows + 2
    idx, val = L.transpose_ref(src, rows, cols, lds, ldt, so, do)
    assert idx.numel() == rows * cols == idx.unique().numel()
    for r in range(rows):
        for c in range(cols):
            k = r * cols + c
            assert int(idx[k]) == do + c * ldt + r
            assert L.same_bits(val[k:k + 1], L.bf16_full(src[so + r * lds + c].reshape(1)))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=R.dname)
def test_feat_ref_is_transpose_and_zero_padding(dtype):
    f = L.special_input((2, 5, 7), 8)
    for pl, pr in ((0, 0), (1, 1), (3, 0), (0, 2)):
        out = L.feat_ref(f, pl, pr, dtype)
        assert out.shape == (2, pl + 7 + pr, 5)
        assert L.same_bits(out[:, pl:pl + 7], L.to_dtype(f.transpose(1, 2).contiguous(), dtype))
        pad = torch.cat([out[:, :pl], out[:, pl + 7:]], 1)
        assert not bool(L.bits(pad).count_nonzero())               # +0, not -0


# ================================================================================================= log-mel
def _logmel_case(frames, nb, nm, kind, cf, mutation=None):
    spec, mel = L.logmel_inputs(frames, nb, nm, kind, 2 * nb + 3)
    ref, s = L.logmel_ref(spec, mel, L.LOGMEL_EPS, cf)
    got = L.logmel_fp32(spec, mel, L.LOGMEL_EPS, cf, mutation)
    return L.check_logmel(got, ref, L.logmel_bound(ref, s, nb)), ref, s


def test_logmel_ref_is_the_formula():
    spec, mel = L.logmel_inputs(3, 5, 4, "gauss", 13)
    for cf in (False, True):
        ref, s = L.logmel_ref(spec, mel, L.LOGMEL_EPS, cf)
        for f in range(3):
            for m in range(4):
                acc = sum((float(spec[f, k]) ** 2 + float(spec[f, 5 + k]) ** 2) * float(mel[k, m]) for k in range(5))
                want = math.log(acc + float(np.float32(1e-6)))
                assert abs(float(ref[m, f] if cf else ref[f, m]) - want) <= 1e-13 * max(1.0, abs(want))


@pytest.mark.parametrize("kind", L.LOGMEL_KINDS)
@pytest.mark.parametrize("frames,nb,nm", L.LOGMEL_SHAPES)
def test_logmel_bound_admits_the_fp32_loop(frames, nb, nm, kind):
    for cf in (False, True):
        r, ref, s = _logmel_case(frames, nb, nm, kind, cf)
        assert r <= 1.0, (frames, nb, nm, kind, cf, r)
        assert bool(torch.isfinite(ref).all()) and float(s.min()) >= L.LOGMEL_EPS
        if kind == "zero":
            assert bool((ref == math.log(L.LOGMEL_EPS)).all())
        if kind == "empty-cols":
            col0 = ref[0] if cf else ref[:, 0]
            assert bool((col0 == math.log(L.LOGMEL_EPS)).all())


def test_logmel_bound_is_tight_enough_to_see_an_fp32_ulp_error_of_the_sum():
    """A relative error of (n_bins + 4) * 2^-22 on the sum - four times what the rounding count allows - is outside."""
    spec, mel = L.logmel_inputs(7, 201, 80, "gauss", 402)
    ref, s = L.logmel_ref(spec, mel, L.LOGMEL_EPS, False)
    off = torch.log(s * (1.0 + 205 * 2.0 ** -22))
    assert L.check_logmel(off, ref, L.logmel_bound(ref, s, 201)) > 1.0


@pytest.mark.parametrize("mutation,kind", [("layout", "gauss"), ("re-for-im", "gauss"), ("no-eps", "zero"), ("no-eps", "empty-cols")])
def test_logmel_mutations_exceed_the_bound(mutation, kind):
    for cf in (False, True):
        r, _, _ = _logmel_case(7, 201, 80, kind, cf, mutation)
        assert r > 1e3, (mutation, kind, cf, r)


# ================================================================================================= dropout
@pytest.mark.parametrize("dtype", [F32, BF16], ids=R.dname)
def test_dropout_expected_is_one_multiply_one_add_one_rounding(dtype):
    rows, cols, p = 9, 14, 0.1
    x, resid = R.to_dtype(R.randn((rows, cols), 81), dtype), R.to_dtype(R.randn((rows, cols), 82), dtype)
    keep = torch.from_numpy(DO.keep_flat(3, rows, cols, 0.5))
    sc = DO.keep_scale(p)
    for res in (None, resid):
        got = L.dropout_expected(x, res, keep, sc, dtype)
        for r in range(rows):
            for c in range(cols):
                v = np.float32(x[r, c].float().item()) * np.float32(sc) if keep[r, c] else np.float32(0.0)
                if res is not None:
                    v = np.float32(v + np.float32(res[r, c].float().item()))
                want = L.to_dtype(torch.tensor([v], dtype=F32), dtype)
                assert L.same_bits(got[r, c].reshape(1), want), (r, c)
        assert got.dtype == dtype
    # the keep scale of a float rate, 1 / (1 - p), is another number: the bits tell
    assert not L.same_bits(L.dropout_expected(x, None, keep, 1.0 / (1.0 - p), F32).float(), L.dropout_expected(x, None, keep, sc, F32).float())


def _drop_thr(p):
    """tmi_drop_thr of csrc/tmi_common.h: (uint32_t)(p * 65536.0f + 0.5f) in fp32; accepted when p < 1 and thr <= 65535."""
    return int(np.float32(np.float32(p) * np.float32(65536.0)) + np.float32(0.5))


def test_rate_table_thresholds_scales_and_refusals():
    for thr, p in L.RATES:
        assert DO.drop_thr(p) == thr == _drop_thr(p), (thr, p)
        assert DO.keep_scale(p) == float(np.float32(65536.0) / np.float32(65536 - thr))
        assert abs(DO.keep_scale(p) - 65536.0 / (65536 - thr)) <= 2.0 ** -24 * 65536.0 / (65536 - thr)
        assert L.drop_ok(p) and p < 1.0 and _drop_thr(p) <= 65535
    assert DO.keep_scale(0.99999) == 65536.0
    assert DO.drop_thr(L.P_OFF) == 0 and L.P_OFF > 0 and L.drop_ok(L.P_OFF)
    assert _drop_thr(0.999995) == 65536 and not L.drop_ok(0.999995)
    assert not L.drop_ok(1.0) and not (np.float32(1.0) < np.float32(1.0))
    assert [L.drop_ok(p) for p in L.P_REFUSED] == [False] * 4


def _conditions(keep, thr, where):
    kept, dropped, sd = L.mask_conditions(keep, thr)
    assert kept >= 1 and dropped >= 1, (where, thr, kept, dropped)
    assert sd <= 5.0, (where, thr, kept, dropped, sd)
    return kept, dropped


@pytest.mark.parametrize("thr,p", L.RATES, ids=L.RATE_IDS)
def test_masks_of_every_gpu_case_hold_kept_and_dropped_elements(thr, p):
    seen = {}
    for rows, cols in L.FLAT_SHAPES:
        seen[(rows, cols)] = _conditions(DO.keep_flat(L.FLAT_SEED, rows, cols, p), thr, ("flat", rows, cols))
    for seed in (L.LN_RATE_SEED_Y, L.LN_RATE_SEED_MASKED):
        _conditions(DO.keep_flat(seed, *L.LN_RATE_SHAPE, p), thr, ("layernorm", hex(seed)))
    for name, (M, N, K, seed) in L.GEMM_RATE_CASES.items():
        _conditions(DO.keep_flat(seed, M, N, p), thr, ("gemm", name))
    for B, H, Tq, Tk, mask, seed in L.ATTN_RATE_CASES:
        seen[(B, H, Tq, Tk)] = _conditions(DO.keep_attention(seed, B, H, Tq, Tk, p), thr, ("attention", B, H, Tq, Tk))
    if thr == 1:        # the counts the shapes were chosen by
        assert seen[(600, 1026)][1] == 17 and seen[(2, 2, 130, 200)][1] == 2
    if thr == 65535:
        assert seen[(600, 1026)][0] == 13 and seen[(2, 2, 130, 200)][0] == 1


@pytest.mark.parametrize("p", L.LAYOUT_DROP_P)
def test_masks_of_the_layout_file_shapes(p):
    thr = DO.drop_thr(p)
    for rows, cols in L.LAYOUT_DROP_SHAPES:
        kept, dropped, sd = L.mask_conditions(DO.keep_flat(L.LAYOUT_DROP_SEED, rows, cols, p), thr)
        assert kept >= 1 and dropped >= 1 and sd <= 5.0, (rows, cols, p, kept, dropped, sd)
