"""The SpecAugment restatement of tests/_spec_augment_ref.py pinned on the host (no GPU): against a literal transcription of
the reference's pad-shift-OR loop (V:1083-1086), on planted starts, and on the start rate of the generator; the site-seed
formula against two hand-computed values; the host validator's refusals, the header / binding of the new entry points, and
the flag errors of speech_jobs/wav2vec2_asr.py."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _spec_augment_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def planted(cols, at, rows=1):
    s = np.zeros((rows, cols), dtype=bool)
    for c in at:
        s[:, c] = True
    return s


@pytest.mark.parametrize("cols", [1, 31, 32, 33, 63, 64, 65, 129, 200])
@pytest.mark.parametrize("length", [1, 2, 10, 32, 33, 64])
@pytest.mark.parametrize("prob", [0.05, 0.5])
def test_spans_equal_the_literal_pad_shift_or_loop(cols, length, prob):
    start = S.starts(S.site_seed(5, 2), S.STREAM_TIME, 4, cols, prob)
    assert np.array_equal(S.spans(start, length), S.spans_literal(start, length))


def test_planted_starts():
    # a single start at column 0
    m = S.spans(planted(40, [0]), 10)
    assert m[0].tolist() == [True] * 10 + [False] * 30
    # a start at cols - 1: the span is cut to one column
    m = S.spans(planted(40, [39]), 10)
    assert m[0].tolist() == [False] * 39 + [True]
    # two overlapping spans: the union, not a sum
    m = S.spans(planted(40, [5, 9]), 10)
    assert m[0].tolist() == [False] * 5 + [True] * 14 + [False] * 21
    # length 1: the mask is the starts
    s = planted(70, [0, 3, 31, 32, 69])
    assert np.array_equal(S.spans(s, 1), s)
    # a span crossing the word edges 31 / 32 and 63 / 64
    m = S.spans(planted(100, [30, 62]), 4)
    assert np.flatnonzero(m[0]).tolist() == [30, 31, 32, 33, 62, 63, 64, 65]
    bits = S.pack_bits(m)
    assert bits.shape == (1, 4) and bits[0].tolist() == [0xC0000000, 0xC0000003, 0x00000003, 0]
    assert np.array_equal(S.unpack_bits(bits, 100), m)
    # the longest span reaches exactly 64 columns, from the last column of the previous 64
    m = S.spans(planted(200, [63]), 64)
    assert np.flatnonzero(m[0]).tolist() == list(range(63, 127))


def test_bit_layout_and_padding():
    m = planted(33, [0, 31, 32], rows=2)
    b = S.pack_bits(m, ld=5)
    assert b.dtype == np.uint32 and b.shape == (2, 5) and b[1].tolist() == [0x80000001, 1, 0, 0, 0]
    assert np.array_equal(S.unpack_bits(b.view(np.int32), 33), m)


@pytest.mark.parametrize("prob", [0.05, 0.5])
def test_start_rate_is_binomial(prob):
    """The starts over a 64 x 4096 grid against Binomial(n, thr / 65536), 6 standard deviations: a statement about the
    generator the arithmetic fixes, not a fitted number."""
    n = 64 * 4096
    q = S.drop_thr(prob) / 65536.0
    for stream in (S.STREAM_TIME, S.STREAM_FEAT):
        k = int(S.starts(S.site_seed(0, 0), stream, 64, 4096, prob).sum())
        sd = math.sqrt(n * q * (1 - q))
        print(f"starts stream {stream} prob {prob}: {k} of {n}, expected {n * q:.1f}, {abs(k - n * q) / sd:.2f} sd")
        assert abs(k - n * q) <= 6 * sd


def test_prob_zero_sets_nothing_and_streams_differ():
    assert not S.starts(S.site_seed(1, 1), S.STREAM_TIME, 3, 100, 0.0).any()
    a, b = S.starts(S.site_seed(1, 1), 1, 8, 256, 0.3), S.starts(S.site_seed(1, 1), 2, 8, 256, 0.3)
    assert not np.array_equal(a, b)
    assert not np.array_equal(a, S.starts(S.site_seed(1, 2), 1, 8, 256, 0.3))
    # the mask of frame t does not depend on how many columns are drawn
    assert np.array_equal(S.time_mask(77, 3, 200, 0.1, 7)[:, :150], S.time_mask(77, 3, 150, 0.1, 7))


def test_site_seed_against_hand_computed_values():
    # 7 * 0xD1B54A32D192ED03 = 105777459947855182613 = 5 * 2^64 + 0xBBF50763BB047B15
    assert 7 * 0xD1B54A32D192ED03 == 105777459947855182613 == 5 * 2 ** 64 + 0xBBF50763BB047B15
    assert S.site_seed(0, 0) == 0xBBF50763BB047B15
    # 3 * 0x9E3779B97F4A7C15 = 34202144457969595455; 1234 + that + the above = 7 * 2^64 + 0x969B749038E3F426
    assert 1234 + 34202144457969595455 + 105777459947855182613 == 7 * 2 ** 64 + 0x969B749038E3F426
    assert S.site_seed(1234, 3) == 0x969B749038E3F426
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2 as w
    assert w.SITE_SPEC == 7 == w.SITE_CTC + 1
    assert w.spec_site_seed(0, 0) == S.site_seed(0, 0) and w.spec_site_seed(1234, 3) == S.site_seed(1234, 3)
    assert w.spec_site_seed(2 ** 64 - 1, 2 ** 40) == S.site_seed(2 ** 64 - 1, 2 ** 40)


def test_dataclass_defaults_and_validator():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2 as w
    s = w.SpecAugment()
    assert (s.mask_time_prob, s.mask_time_length, s.mask_feature_prob, s.mask_feature_length) == (0.05, 10, 0.0, 10)
    assert w.check_spec_augment_args(s, 249, 768) == (True, False)
    assert w.check_spec_augment_args(w.SpecAugment(0.0, 1, 0.999, 64), 1, 8) == (False, True)
    bad = [(dict(mask_time_prob=-0.01), "mask_time_prob"), (dict(mask_time_prob=1.0), "mask_time_prob"),
           (dict(mask_time_prob=0.999999), "mask_time_prob"), (dict(mask_time_prob=float("nan")), "mask_time_prob"),
           (dict(mask_feature_prob=1.5), "mask_feature_prob"), (dict(mask_time_length=0), "mask_time_length <= 64"),
           (dict(mask_time_length=65), "mask_time_length <= 64"), (dict(mask_feature_length=65), "mask_feature_length <= 64"),
           (dict(mask_feature_length=2.5), "mask_feature_length"), (dict(mask_time_prob="0.1"), "mask_time_prob")]
    for kw, needle in bad:
        with pytest.raises(ValueError, match=re.escape(needle)):
            w.check_spec_augment_args(w.SpecAugment(**kw), 100, 768)
    for T, H, needle in ((0, 768, "4096"), (4097, 768, "4096"), (100, 12, "multiple of 8"), (100, 4104, "multiple of 8")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            w.check_spec_augment_args(s, T, H)
    with pytest.raises(TypeError):
        w.check_spec_augment_args(dict(mask_time_prob=0.05), 100, 768)
    # the reference's names, argument order and defaults (V:1073, V:1098), with seed / step in place of TF's global stream
    import inspect
    for fn in (w.apply_time_mask, w.apply_feature_mask):
        p = inspect.signature(fn).parameters
        assert list(p) == ["hidden_states", "mask_prob", "mask_length", "seed", "step"]
        assert (p["mask_prob"].default, p["mask_length"].default, p["seed"].default, p["step"].default) == (0.05, 10, 0, 0)
    for fn in (w.Wav2Vec2ForCTC.head_step, w.fit_ctc_head):
        assert inspect.signature(fn).parameters["spec_augment"].default is None
    assert "spec_augment" not in inspect.signature(w.Wav2Vec2ForSequenceClassification.head_step).parameters


def test_header_and_binding_of_the_new_entry_points():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib
    header = open(os.path.join(ROOT, "include", "tethys_mi.h")).read()
    sig = _lib.SIGNATURES
    for name in ("tmi_spec_masks", "tmi_span_mask_apply", "tmi_ctc_head_fwd_m", "tmi_ctc_head_bwd_m", "tmi_layer_mix_bwd_m"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/tethys_mi.h"
        assert name in sig and len(sig[name][1]) == m.group(1).count(",") + 1, name
    for name in ("tmi_ctc_head_fwd", "tmi_ctc_head_bwd", "tmi_layer_mix_bwd"):
        assert len(sig[name + "_m"][1]) == len(sig[name][1]) + 4
    assert "SITE_SPEC = 7" in header
    h = _lib.lib()   # binds every declared symbol
    assert h.tmi_abi_version() == _lib.ABI_VERSION
    # the host refusals need no device: nothing is launched
    for args in ((None, 1, None, 1, None, 1, 32, 8, 0.05, 10, 0.05, 10, 0, None),        # both masks NULL
                 (4096, 0, None, 1, None, 1, 32, 8, 0.05, 10, 0.05, 10, 0, None),        # ld_t too small
                 (4096, 1, None, 1, None, 1, 32, 8, 0.05, 65, 0.05, 10, 0, None),        # length 65
                 (4096, 1, None, 1, None, 1, 32, 8, 1.0, 10, 0.05, 10, 0, None),         # prob 1
                 (4096, 1, None, 1, None, 0, 32, 8, 0.05, 10, 0.05, 10, 0, None),        # N 0
                 (4098, 1, None, 1, None, 1, 32, 8, 0.05, 10, 0.05, 10, 0, None)):       # misaligned
        assert h.tmi_spec_masks(*args) == -1
        assert h.tmi_last_error().decode().startswith("tmi_spec_masks:") and "length <= 64" in h.tmi_last_error().decode()


def _job(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "speech_jobs", "wav2vec2_asr.py"), *flags], capture_output=True,
                          text=True, timeout=300)


@pytest.mark.parametrize("flags, needle", [
    (["--mask_time_prob", "0.1"], "--mask_time_prob comes with --fit_head"),
    (["--mask_feature_length", "4", "--labels", "x"], "--mask_feature_length comes with --fit_head"),
    (["--fit_head", "--labels", "x", "--mask_time_length", "65"], "1 <= mask_time_length <= 64"),
    (["--fit_head", "--labels", "x", "--mask_feature_prob", "1.0"], "mask_feature_prob must be in [0, 1)"),
    (["--fit_head", "--labels", "x", "--mask_time_prob", "abc"], "invalid float value"),
])
def test_job_flag_errors(flags, needle):
    r = _job(*flags)
    assert r.returncode == 2 and needle in r.stderr, r.stderr
