"""Sampled decoding, host side (no GPU): ``check_sample_args``, the draw bits against values worked out with plain
integers, both choice rules of tests/_sample_ref.py against the distribution they claim to sample (chi-square on fixed
seeds), the rule's edge cases and the transcription job's new flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _sample_ref as R
from _margins import within

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _whisper():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import whisper
    return whisper


def test_check_sample_args_bounds_and_defaults():
    w = _whisper()
    cfg = w.make_config("tiny")
    assert w.check_sample_args(cfg) == cfg.max_target_positions
    assert w.sample_args(cfg, 10) == (10, 50, 1.0, 0)  # top_k None -> 50, top_p None -> 1, min_length None -> 0
    assert w.sample_args(cfg, 10, 1, 0.5, 0, None, 10) == (10, 0, 1.0, 10)
    assert w.sample_args(cfg, 10, None, 2.0, 64, 0.25, 3) == (10, 64, 0.25, 3)
    for bad in (dict(num_beams=2), dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")),
                dict(top_k=65), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=0, top_p=0.9),
                dict(min_length=-1), dict(min_length=11), dict(max_length=cfg.max_target_positions + 1)):
        with pytest.raises(ValueError):
            w.check_sample_args(cfg, **{"max_length": 10, **bad})
    assert w.sample_step_seed(5, 0) == 5
    assert w.sample_step_seed(2 ** 64 - 1, 1) == 0x9E3779B97F4A7C14
    assert w.sample_step_seed(5, 3) == R.step_seed(5, 3)


def test_sample_bits_match_hand_computed_values():
    # mix32(rk.a ^ mix32(c ^ rk.b)), rk = row_key(stream_key(seed, 0), row), worked out with plain Python integers
    for (seed, row, col), want in (((0, 0, 0), 0x8A06EB4A), ((1, 2, 3), 0x47D04EA1),
                                   ((0x123456789ABCDEF, 40, 51864), 0x8E4A49AC), ((7, 5, 0xFFFFFFFF), 0x71B3D776),
                                   ((2 ** 64 - 1, 16, 128), 0x058BB128)):
        assert int(R.sample_bits(seed, row, col)) == want
    u = R.uniform(np.array([0, 0xFFFFFFFF, 0x80000000], dtype=np.uint64))
    assert u.tolist() == [2.0 ** -25, 1 - 2.0 ** -25, 0.5 + 2.0 ** -25]


_SCORES = np.log(np.array([0.30, 0.22, 0.15, 0.12, 0.09, 0.06, 0.04, 0.02]))[::-1].copy() + 1.25  # (unsorted on purpose)
# the 0.999 quantiles of chi-square with 7 and 4 degrees of freedom
_CHI2_999 = {7: 24.322, 4: 18.467}


def _counts(mode, **kw):
    """Tokens of 64 seeds x 64 rows (4096 draws) of one score vector."""
    counts = np.zeros(8)
    for seed in range(64):
        s, lse, top = R.rank(np.tile(_SCORES, (64, 1)))
        if mode == "gumbel":
            tok = R.choose_gumbel(s, lse, 1000 + seed)[0]
        else:
            tok = R.choose_topk(s, lse, top, 1000 + seed, **kw)[0]
        counts += np.bincount(tok, minlength=8)
    return counts


def _chi2(counts, p):
    keep = p > 0
    assert counts[~keep].sum() == 0
    e = p[keep] * counts.sum()
    return float((((counts[keep] - e) ** 2) / e).sum())


def test_both_modes_sample_the_stated_distribution():
    p = np.exp(_SCORES - np.log(np.exp(_SCORES).sum()))
    assert _chi2(_counts("gumbel"), p) < _CHI2_999[7]
    assert _chi2(_counts("topk", top_k=8, top_p=1.0), p) < _CHI2_999[7]
    # top_k 5: the five largest, renormalised
    p5 = np.where(p >= np.sort(p)[-5], p, 0.0)
    assert _chi2(_counts("topk", top_k=5, top_p=1.0), p5 / p5.sum()) < _CHI2_999[4]


def test_rule_edge_cases():
    rng = np.random.RandomState(3)
    s0 = rng.randn(32, 300) * 2
    s, lse, top = R.rank(s0)
    tok, lp, decided, _ = R.choose_topk(s, lse, top, 9, 1, 1.0)
    assert np.array_equal(tok, s0.argmax(1)) and decided.all()  # top_k = 1 is the argmax
    assert np.allclose(lp, s0.max(1) - lse)
    tok, _, _, _ = R.choose_topk(s, lse, top, 9, 50, 1e-6)
    assert np.array_equal(tok, s0.argmax(1))  # top_p so small that m = 1
    # the nucleus: only the candidates up to the first running sum >= top_p of the top-k mass are drawn
    for seed in range(20):
        tok, _, _, _ = R.choose_topk(s, lse, top, seed, 10, 0.5)
        for r in range(32):
            p = np.exp(s[r, top[r, :10]] - lse[r])
            m = int(np.argmax(np.cumsum(p) >= 0.5 * p.sum())) + 1
            assert tok[r] in top[r, :m]
    # a suppressed column is never drawn, although it is the largest score of every row
    s1 = s0.copy()
    s1[:, 17] = 50.0
    sS, lseS, topS = R.rank(s1, suppress_id=17)
    for seed in range(20):
        assert 17 not in R.choose_topk(sS, lseS, topS, seed, 50, 1.0)[0]
        assert 17 not in R.choose_gumbel(sS, lseS, seed)[0]
    # equal scores: the smaller column first
    sT, lseT, topT = R.rank(np.zeros((4, 10)))
    assert R.choose_topk(sT, lseT, topT, 0, 1, 1.0)[0].tolist() == [0, 0, 0, 0]


def test_exact_score_inputs_meet_the_undecided_cap_and_the_margins_are_measured():
    """The GPU test's exact-score inputs and seeds, from the restatement alone: every (M, T, top_k, top_p / Gumbel)
    configuration has at most 1 % of its rows undecided.  And the b = 0 margins next to what fp32 arithmetic does to
    the same inputs (numpy's float32 in the kernel's order of operations)."""
    p_err = g_err = 0.0
    for M in R.EXACT_MS:
        for T in R.EXACT_TS:
            s, lse, top = R.exact_ranked(M, T)
            assert float(np.abs(lse).max()) < 32
            p_err = max(p_err, float(R.running_sum_error_fp32(s, lse, top, 64).max()))
            g_err = max(g_err, float(R.gumbel_error_fp32(s, R.exact_seed(M, T, 0, 1.0)).max()))
            for top_k, top_p in R.EXACT_KP:
                dec = R.exact_choice(M, T, top_k, top_p)[2]
                assert R.cap_ok(dec, R.EXACT_CAP), (M, T, top_k, top_p, int((~dec).sum()))
    within("sample rule: running sums in fp32 against fp64, relative to the candidates' mass", p_err, R.P_SUM_TOL)
    within("sample rule: s + g in fp32 against fp64", g_err, R.G_TOL)


@pytest.mark.parametrize("wdt", ["bf16", "fp32"])
def test_random_inputs_meet_the_undecided_cap(wdt):
    """The GPU test's LayerNorm inputs and seeds: at most 10 % of every configuration's rows undecided at the top-k
    test's bound b."""
    for d in R.RANDOM_DS:
        refs = R.random_inputs(wdt, d)[4]
        for M in R.RANDOM_MS:
            for top_k, top_p in R.RANDOM_KP:
                dec = R.random_choice(refs[M], wdt, d, M, top_k, top_p)[2]
                assert R.cap_ok(dec, R.RANDOM_CAP), (wdt, d, M, top_k, top_p, int((~dec).sum()))


def test_transcribe_job_rejects_sampling_with_beams():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "speech_jobs", "whisper_transcribe.py"), "--do_sample",
                        "--num_beams", "2"], capture_output=True, text=True)
    assert r.returncode == 2 and "--do_sample" in r.stderr
