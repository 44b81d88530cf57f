"""Greedy decoding, host side (no GPU): the stop rule and the one-step-late EOS read of ``whisper.greedy_loop``, the
argument checks of ``generate`` (W:636-648 and the fixed reference bugs), the wav reader and the transcription job's CLI."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _whisper():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import whisper
    return whisper


class FakeDecoder:
    """A token table [max_length + 1, rows] standing in for the device: step(t) 'computes' row t, read_eos(t) counts EOS
    there, but only once step t has been queued."""

    def __init__(self, table, eos=2):
        self.table, self.eos = np.asarray(table), eos
        self.queued, self.read = [], []

    def step(self, t):
        assert t == len(self.queued) + 1, "steps are queued in order"
        self.queued.append(t)

    def read_eos(self, t):
        assert t in self.queued, "a count is read only after its step was queued"
        self.read.append(t)
        return int((self.table[t] == self.eos).sum())


def _run(table, max_length, late=True, eos=2):
    w = _whisper()
    f = FakeDecoder(table, eos)
    n = w.greedy_loop(max_length, f.table.shape[1], f.step, f.read_eos, late=late)
    return n, f


def test_stops_only_on_an_all_eos_step():
    rows, L = 3, 10
    table = np.full((L + 1, rows), 7)
    table[2, 0] = 2           # row 0 emits EOS early: it keeps decoding
    table[4, :2] = 2          # two of three rows: no stop
    table[6, :] = 2           # every row in the same step: stop after step 6
    table[8, :] = 2
    n, f = _run(table, L)
    assert n == 6
    n_sync, _ = _run(table, L, late=False)
    assert n_sync == 6


def test_rows_with_an_earlier_eos_keep_going_to_max_length():
    rows, L = 2, 12
    table = np.full((L + 1, rows), 5)
    table[3, 0] = 2
    table[5, 1] = 2  # each row emits EOS once, never in the same step
    n, f = _run(table, L)
    assert n == L and f.queued == list(range(1, L + 1))


@pytest.mark.parametrize("stop_at", [None, 1, 2, 7, 20])
def test_late_read_truncates_like_a_synchronous_read(stop_at):
    rows, L = 4, 20
    rng = np.random.default_rng(stop_at or 0)
    table = rng.integers(0, 6, size=(L + 1, rows))
    table[table == 2] = 3
    if stop_at is not None:
        table[stop_at, :] = 2
    n_late, f_late = _run(table, L, late=True)
    n_sync, f_sync = _run(table, L, late=False)
    assert n_late == n_sync == (stop_at if stop_at is not None else L)
    # the late loop queues at most one step beyond the one that stopped it (its column is dropped by the truncation)
    assert f_sync.queued == list(range(1, n_sync + 1))
    assert f_late.queued[:n_late] == f_sync.queued and len(f_late.queued) <= min(L, n_late + 1)
    assert max(f_late.read) == n_late


def test_no_stop_check_without_eos():
    w = _whisper()
    queued = []
    assert w.greedy_loop(5, 3, queued.append, None) == 5 and queued == [1, 2, 3, 4, 5]
    assert w.greedy_loop(0, 3, queued.append, None) == 0


def test_generate_argument_bounds():
    w = _whisper()
    cfg = w.make_config("small")
    assert w.check_generate_args(cfg) == 448
    for ml in (0, 1, 448):
        assert w.check_generate_args(cfg, ml) == ml
    for bad in (dict(max_length=449), dict(max_length=-1), dict(num_beams=2), dict(temperature=0.0),
                dict(temperature=-1.0)):
        with pytest.raises(ValueError):
            w.check_generate_args(cfg, **bad)
    # accepted and ignored, as in the reference
    assert w.check_generate_args(cfg, 10, num_beams=1, temperature=0.7) == 10


def _write_wav(path, samples, rate=16000, width=2, channels=1):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(samples.tobytes())


def test_read_wav(tmp_path):
    w = _whisper()
    pcm = (np.sin(np.arange(1600) * 0.05) * 12000).astype("<i2")
    p = tmp_path / "a.wav"
    _write_wav(p, pcm)
    got = w.read_wav(str(p))
    assert got.dtype == np.float32 and got.shape == (1600,)
    assert np.array_equal(got, pcm.astype(np.float32) / 32768.0)
    _write_wav(tmp_path / "b.wav", pcm, rate=8000)
    _write_wav(tmp_path / "c.wav", np.repeat(pcm, 2), channels=2)
    for bad in ("b.wav", "c.wav"):
        with pytest.raises(ValueError):
            w.read_wav(str(tmp_path / bad))


def test_dummy_waveform_is_seeded_30s():
    w = _whisper()
    a, b = w.dummy_waveform(), w.dummy_waveform()
    assert a.shape == (480000,) and a.dtype == np.float32 and np.array_equal(a, b)


def test_transcribe_job_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "speech_jobs", "whisper_transcribe.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--model_type", "--precision", "--resume_from", "--wav", "--batch_size", "--max_length"):
        assert flag in r.stdout
