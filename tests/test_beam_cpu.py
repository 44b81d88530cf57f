"""Beam search, host side (no GPU): the decoding rule as restated in tests/_beam_ref.py on hand-built log-probability
tables (beam beats greedy, EOS below and at/above rank K, the pool's strict replacement, both early_stopping modes,
length penalties, disabled EOS), the argument checks of ``check_beam_args`` and the transcription job's new flags."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _beam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
START, EOS = 4, 2
NEG = -np.inf


def _whisper():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import whisper
    return whisper


def _by_last_token(table):
    """lp_fn whose row depends on the prefix's last token: log(table[last])."""
    lt = {k: np.log(np.asarray(v, dtype=np.float64)) for k, v in table.items()}
    return lambda prefixes: [lt[p[-1]] for p in prefixes]


def _cands(rows, N):
    """[(ids, lps)] per row -> numpy candidate tables [rows, N]."""
    ids = np.array([r[0] for r in rows], dtype=np.int64)
    lps = np.array([r[1] for r in rows], dtype=np.float32)
    assert ids.shape[1] == N
    return ids, lps


def test_beam_finds_a_better_sequence_than_greedy():
    # token 1 is the likelier first token, but every continuation after it is poor; token 3 leads to a sure token 0
    table = {START: [0.04, 0.5, 0.02, 0.4, 0.04], 1: [0.34, 0.1, 0.33, 0.13, 0.1], 3: [0.94, 0.02, 0.02, 0.01, 0.01],
             0: [0.2] * 5, 2: [0.2] * 5}
    lp = _by_last_token(table)
    greedy = [START]
    for _ in range(2):
        greedy.append(int(np.argmax(lp([greedy])[0])))
    assert greedy == [START, 1, 0]
    greedy_lp = math.log(0.5) + math.log(0.34)
    ref = R.run(lp, B=1, K=2, max_length=2, start=START, eos=-1, length_penalty=0.0)
    seqs, scores, lens = ref.output(2)
    assert seqs[0] == [START, 3, 0] and lens == [2, 2]
    assert scores[0] == pytest.approx(math.log(0.4) + math.log(0.94)) and scores[0] > greedy_lp
    assert scores[0] >= scores[1]


def test_eos_below_rank_k_is_offered_and_at_rank_k_or_above_skipped():
    K, N = 2, 4
    ref = R.BeamRef(1, K, 8, start=START, eos=EOS, length_penalty=1.0)
    # step 1: beam 1 is -inf, so the ranks are beam 0's: 5, EOS, 7, 9 -> EOS at rank 1 < K is offered
    ids, lps = _cands([([5, EOS, 7, 9], [-0.1, -0.5, -1.0, -2.0]), ([5, EOS, 7, 9], [-0.1, -0.5, -1.0, -2.0])], N)
    ref.step(ids, lps)
    assert [e[2] for e in ref.pools[0]] == [[START, EOS]] and ref.pools[0][0][0] == np.float32(-0.5)
    assert ref.prefix == [[START, 5], [START, 7]]
    assert ref.sums == [np.float32(-0.1), np.float32(-1.0)]
    # step 2: EOS only at ranks 2 and 3 (>= K): skipped, the pool keeps one entry
    ids, lps = _cands([([6, 8, EOS, 9], [-0.1, -0.2, -3.0, -4.0]), ([EOS, 6, 8, 9], [-2.5, -3.0, -3.1, -3.2])], N)
    ref.step(ids, lps)
    assert len(ref.pools[0]) == 1
    assert ref.prefix == [[START, 5, 6], [START, 5, 8]]
    assert not ref.done[0]


def test_pool_replacement_is_strict_and_ordered():
    K = 2
    ref = R.BeamRef(1, K, 8, start=START, eos=EOS)
    ref._offer(0, np.float32(-2.0), [START, 9, EOS])
    ref._offer(0, np.float32(-1.0), [START, 8, EOS])
    assert [e[0] for e in ref.pools[0]] == [np.float32(-1.0), np.float32(-2.0)]
    ref._offer(0, np.float32(-2.0), [START, 7, EOS])  # equal to the worst: not admitted
    assert [e[2][1] for e in ref.pools[0]] == [8, 9]
    ref._offer(0, np.float32(-1.0), [START, 6, EOS])  # strictly greater than the worst: replaces it, after the equal one
    assert [e[2][1] for e in ref.pools[0]] == [8, 6]
    # while the pool is not full, ties keep insertion order
    ref2 = R.BeamRef(1, 3, 8, start=START, eos=EOS)
    for tok in (5, 6, 7):
        ref2._offer(0, np.float32(-1.0), [START, tok, EOS])
    assert [e[2][1] for e in ref2.pools[0]] == [5, 6, 7]


def _two_eos_steps(early, length_penalty=1.0):
    K, N = 2, 4
    ref = R.BeamRef(1, K, 8, start=START, eos=EOS, length_penalty=length_penalty, early_stopping=early)
    ids, lps = _cands([([EOS, 5, 7, 9], [-0.1, -0.5, -1.0, -2.0])] * 2, N)
    ref.step(ids, lps)  # EOS at rank 0: pool [START, EOS]; live 5, 7
    ids, lps = _cands([([EOS, 6, 8, 9], [-0.2, -0.3, -3.0, -4.0]), ([6, 8, 9, EOS], [-0.1, -0.2, -0.3, -5.0])], N)
    ref.step(ids, lps)  # EOS of beam 0 at rank 0 (score -0.7): the pool is full
    return ref


def test_early_stopping_modes():
    ref = _two_eos_steps(True)
    assert len(ref.pools[0]) == 2 and ref.done[0] and ref.n_done == 1
    ref = _two_eos_steps(False)
    # best live sum after step 2: -0.5 - 0.3 = -0.8, / 2 = -0.4 > the worst pool score -0.35? no: -0.35 >= -0.4 -> done
    worst = ref.pools[0][-1][0]
    best_live = max(ref.sums)
    assert ref.done[0] == bool(worst >= np.float32(best_live / np.float32(2.0)))
    assert ref.done[0]
    # a live beam that may still win keeps the item going
    K, N = 2, 4
    ref = R.BeamRef(1, K, 8, start=START, eos=EOS, early_stopping=False)
    ids, lps = _cands([([5, EOS, 7, 9], [-0.01, -0.02, -0.03, -4.0])] * 2, N)
    ref.step(ids, lps)  # EOS at rank 1: pool [-0.02]
    ids, lps = _cands([([6, EOS, 8, 9], [-0.001, -0.002, -3.0, -5.0]), ([8, 9, 6, EOS], [-0.001, -0.1, -0.2, -5.0])], N)
    ref.step(ids, lps)  # EOS at rank 1 again: the pool is full, its worst -0.02 < the best live -0.011 / 2
    assert len(ref.pools[0]) == 2 and not ref.done[0]
    frozen = _two_eos_steps(True)
    state = (list(frozen.sums), [list(p) for p in frozen.prefix], [list(e) for e in frozen.pools[0]])
    ids, lps = _cands([([EOS, 6, 8, 9], [-0.0, -0.0, -0.0, -0.0])] * 2, N)
    frozen.step(ids, lps)  # a step after the item is done changes nothing
    assert (list(frozen.sums), [list(p) for p in frozen.prefix], [list(e) for e in frozen.pools[0]]) == state


@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.0])
def test_length_penalty_divides_by_length_power(length_penalty):
    ref = _two_eos_steps(True, length_penalty)
    got = {tuple(e[2]): e[0] for e in ref.pools[0]}
    s1 = np.float32(-0.1)
    s2 = np.float32(np.float32(-0.5) + np.float32(-0.2))
    assert got[(START, EOS)] == np.float32(s1 / np.float32(1.0 ** length_penalty))
    assert got[(START, 5, EOS)] == np.float32(s2 / np.float32(2.0 ** length_penalty))


def test_disabled_eos_runs_to_max_length_and_finalizes():
    table = {t: [0.3, 0.1, 0.4, 0.1, 0.04, 0.03, 0.02, 0.01] for t in range(8)}
    ref = R.run(_by_last_token(table), B=2, K=3, max_length=4, start=START, eos=-1, dtype=np.float64)
    assert ref.t == 4 and not any(ref.done)
    for b in range(2):
        assert len(ref.pools[b]) == 3
        assert all(len(e[2]) == 5 for e in ref.pools[b])
        assert [e[0] for e in ref.pools[b]] == sorted([e[0] for e in ref.pools[b]], reverse=True)
    # with EOS on, token 2 (the likeliest) ends hypotheses at once
    ref = R.run(_by_last_token(table), B=1, K=3, max_length=4, start=START, eos=EOS, dtype=np.float64)
    assert ref.pools[0][0][2] == [START, EOS]


def test_check_beam_args_bounds():
    w = _whisper()
    cfg = w.make_config("small")
    assert w.check_beam_args(cfg, None, 2) == cfg.max_target_positions
    assert w.check_beam_args(cfg, 10, 8, 0.7, 2.0, 8) == 10
    assert w.check_beam_args(cfg, 0, 5, 1.0, 0.0, 1) == 0
    assert w.check_beam_args(cfg, 2, 3, 1.0, 20.0) == 2  # (2 ** 20 is a finite fp32 value; 448 ** 20 is not)
    assert w.check_beam_args(cfg, 448, 3, 1.0, -2.0) == 448
    for kw in (dict(num_beams=1), dict(num_beams=9), dict(num_beams=3, num_return_sequences=4),
               dict(num_beams=3, num_return_sequences=0), dict(num_beams=3, length_penalty=float("inf")),
               dict(num_beams=3, length_penalty=float("nan")), dict(num_beams=3, max_length=449),
               dict(num_beams=3, max_length=-1), dict(num_beams=3, temperature=0.0),
               dict(num_beams=3, max_length=448, length_penalty=20.0), dict(num_beams=3, max_length=448, length_penalty=-20.0),
               dict(num_beams=3, max_length=448, length_penalty=1e300)):
        with pytest.raises(ValueError):
            w.check_beam_args(cfg, **kw)
    with pytest.raises(ValueError):  # the greedy checks are unchanged
        w.check_generate_args(cfg, 10, 2)


def test_transcribe_job_help_lists_beam_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "speech_jobs", "whisper_transcribe.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--num_beams", "--length_penalty", "--num_return_sequences"):
        assert flag in r.stdout, flag
