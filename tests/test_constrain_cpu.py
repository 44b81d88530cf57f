"""Decode constraints without a GPU: ``whisper.check_constraint_args``' every refusal, tests/_constrain_ref.py against
brute-force loops on tiny cases, the teeth of the GPU kernel tests (every listed mutation of the reference changes the
expected result of one of THEIR inputs), the undecided-row caps of the seeds those tests use, and the binding of the four
new entry points in the built library."""
import itertools
import math

import numpy as np
import pytest

import _constrain_ref as R


def _whisper():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import whisper
    return whisper


def _cfg(**kw):
    w = _whisper()
    base = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, encoder_layers=1,
                decoder_layers=1, vocab_size=160, max_target_positions=32, decoder_start_token_id=150)
    base.update(kw)
    return w.make_config("small", **base)


# ----------------------------------------------------------------------------- 1. the validator
def test_defaults_mean_no_constraint():
    w, cfg = _whisper(), _cfg()
    assert w.check_constraint_args(cfg, 10, None) is None
    assert w.check_constraint_args(cfg, None, 3, repetition_penalty=1.0, no_repeat_ngram_size=0, suppress_tokens=[],
                                   begin_suppress_tokens=[], prompt_ids=None) is None


def test_accepted_arguments_come_back_normalised():
    w, cfg = _whisper(), _cfg()
    c = w.check_constraint_args(cfg, 10, None, repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[5, 3, 5],
                                begin_suppress_tokens=(7,), prompt_ids=[[1, 2, 3], [4, 5, 6]])
    assert c["penalty"] == 1.3 and c["ngram"] == 2 and c["suppress"] == [3, 5] and c["begin"] == [7] and c["P"] == 3
    assert c["prompt"].dtype == np.int32 and c["prompt"].shape == (2, 3) and c["max_length"] == 10 and c["active"]
    c = w.check_constraint_args(cfg, None, None, prompt_ids=[1, 2])
    assert c["P"] == 2 and c["max_length"] == 30 and not c["active"]
    assert w.check_constraint_args(cfg, None, None, prompt_ids=[1, 2], return_token_timestamps=True)["max_length"] == 29
    assert np.array_equal(w.token_bitset([0, 31, 32, 159], 160).view(np.uint32), R.bitset([0, 31, 32, 159], 160))


@pytest.mark.parametrize("kw", [
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=math.inf),
    dict(repetition_penalty=math.nan),
    dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=33), dict(no_repeat_ngram_size=2.5),
    dict(suppress_tokens=[160]), dict(suppress_tokens=[-1]), dict(suppress_tokens=[[1, 2]]), dict(suppress_tokens=[1.5]),
    dict(begin_suppress_tokens=[160]), dict(begin_suppress_tokens=[-3]),
    dict(prompt_ids=[160]), dict(prompt_ids=[-1]), dict(prompt_ids=[]), dict(prompt_ids=[[[1]]]), dict(prompt_ids=[0.5]),
    dict(prompt_ids=list(range(23))),                                # P + max_length = 33 > 32
    dict(prompt_ids=list(range(22)), return_token_timestamps=True),  # one less with timestamps
    dict(prompt_ids=list(range(33)), max_length=None),               # no position left at all
    dict(suppress_tokens=[v for v in range(160) if v != 2]),         # with EOS (2) nothing is left
    dict(suppress_tokens=list(range(130)), begin_suppress_tokens=list(range(130, 152)), no_repeat_ngram_size=2),
    dict(suppress_tokens=list(range(155)), num_beams=3),             # 160 - 155 (EOS among them) = 5 < 2 * 3
], ids=lambda kw: ",".join(f"{k}={str(v)[:14]}" for k, v in kw.items()))
def test_every_refusal(kw):
    w, cfg = _whisper(), _cfg()
    kw = dict(kw)
    max_length, num_beams = kw.pop("max_length", 10), kw.pop("num_beams", None)
    with pytest.raises(ValueError):
        w.check_constraint_args(cfg, max_length, num_beams, **kw)


def test_the_free_column_count_is_exact():
    """One column more than the refusals above need, and the call passes; the vocabulary bound of the set builder."""
    w, cfg = _whisper(), _cfg()
    assert cfg.eos_token_id == 2
    assert w.check_constraint_args(cfg, 10, None, suppress_tokens=[v for v in range(159) if v != 7]) is not None  # 7 is left
    assert w.check_constraint_args(cfg, 10, 3, suppress_tokens=list(range(3, 156))) is not None                  # 160 - 153 - 1 = 6
    assert w.check_constraint_args(cfg, 10, None, suppress_tokens=list(range(3, 151)), no_repeat_ngram_size=2) is not None
    with pytest.raises(ValueError):
        w.check_constraint_args(cfg, 10, None, suppress_tokens=list(range(3, 152)), no_repeat_ngram_size=2)       # 160-149-1-10 = 0
    big = _cfg(vocab_size=65537)
    assert w.check_constraint_args(big, 10, None, prompt_ids=[1]) is not None  # (a prompt alone builds no set)
    with pytest.raises(ValueError):
        w.check_constraint_args(big, 10, None, no_repeat_ngram_size=2)


# ----------------------------------------------------------------------------- 2. the reference against brute force
def _brute_sets(row, V, static, ngram):
    """The rule read off the header, token by token: x is banned if appending it makes the last n-gram one that the
    prefix already holds."""
    seen = {x for x in row if 0 <= x < V}
    banned = set(static)
    if ngram >= 1:
        for x in range(V):
            new = tuple(row + [x])[len(row) + 1 - ngram:] if len(row) + 1 >= ngram else None
            if new is None or len(new) != ngram:
                continue
            if any(tuple(row[i:i + ngram]) == new for i in range(len(row) - ngram + 1)):
                banned.add(x)
    return seen, banned


@pytest.mark.parametrize("ngram", [0, 1, 2, 3, 4])
def test_set_builder_equals_brute_force(ngram):
    V = 5
    for t in range(1, 7):
        for row in itertools.product(range(3), repeat=t):
            row = list(row)
            static = [4] if t % 2 else []
            seen, banned = R.build_sets([row], t, V, R.bitset(static, V), ngram)
            s2, b2 = _brute_sets(row, V, static, ngram)
            assert set(np.nonzero(R.to_bool(seen[0], V))[0]) == s2, (row, ngram)
            assert set(np.nonzero(R.to_bool(banned[0], V))[0]) == b2, (row, ngram)
    # ids outside [0, V) set no bit and still take part in the comparison of the contexts
    row = [7, -1, 2, 7, -1]
    seen, banned = R.build_sets([row], 5, V, None, 3)
    assert set(np.nonzero(R.to_bool(seen[0], V))[0]) == {2} and set(np.nonzero(R.to_bool(banned[0], V))[0]) == {2}


def test_constrained_logit_and_choices_on_tiny_rows():
    z = np.array([[3.0, -2.0, 0.0, 1.0, 5.0], [1.0, 2.0, 3.0, 4.0, 5.0]])
    seen, banned = np.stack([R.bitset([0, 1, 2], 5), R.bitset([], 5)]), np.stack([R.bitset([4], 5), R.bitset(range(5), 5)])
    zp = R.constrain(z, seen, banned, 2.0)
    assert np.array_equal(zp[0], [1.5, -4.0, 0.0, 1.0, -np.inf]) and np.all(np.isneginf(zp[1]))
    assert np.array_equal(R.constrain(z, None, None, 2.0), z)
    tok, dec = R.argmax_ref(zp)
    assert list(tok) == [0, 0] and dec.all()
    ids, lp, lse, _ = R.topk_ref(zp, 3)
    assert list(ids[0]) == [0, 3, 2] and list(ids[1]) == [0, 1, 2] and np.isneginf(lse[1]) and np.all(np.isneginf(lp[1]))
    assert abs(lse[0] - math.log(sum(math.exp(v) for v in (1.5, -4.0, 0.0, 1.0)))) < 1e-12 and not np.isnan(lp).any()
    tok, lp, dec, _ = R.sample_ref(zp, 1, 2, 1.0, finished=[0, 0], pad_id=9)
    assert tok[0] in (0, 3) and tok[1] == 9 and lp[1] == 0.0
    tok, lp, _, _ = R.sample_ref(zp, 1, 2, 1.0, finished=[1, 0], pad_id=9)
    assert tok[0] == 9 and lp[0] == 0.0
    # the bound: a larger penalty in either direction widens it, and it never falls below the unconstrained one
    assert np.all(R.constrained_bound(1e-6, zp, 2.0) >= 2e-6) and np.all(R.constrained_bound(1e-6, zp, 0.5) >= 2e-6)
    assert np.all(R.constrained_bound(1e-6, zp, 1.0) >= 1e-6)


# ----------------------------------------------------------------------------- 3. the GPU tests have teeth
def _sets_differ(mutation):
    for c in R.set_cases():
        a, b = R.set_case_expected(c), R.set_case_expected(c, mutation)
        if not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])):
            return True
    return False


def _heads_differ(mutation):
    n = 0
    for d, V, M, p in itertools.product(R.HEAD_DS[:1], R.HEAD_VS, R.HEAD_MS, R.HEAD_PENALTIES):
        a, b = R.head_expected(d, V, M, p), R.head_expected(d, V, M, p, mutation)
        n += int(not np.array_equal(a["argmax"][0], b["argmax"][0]))
        n += int(not np.array_equal(a["topk"][0], b["topk"][0]))
        n += int(not np.array_equal(a["zp"], b["zp"]))
    return n > 0


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_changes_an_expected_result(mutation):
    changed = _heads_differ(mutation) if mutation.startswith("penalty") else _sets_differ(mutation)
    if mutation in R.EQUIVALENT:
        assert not changed, "0 / p and 0 * p differ?"
        return
    assert changed, f"no input of the GPU kernel tests tells {mutation} from the rule"


def test_set_cases_cover_what_they_claim():
    cases = list(R.set_cases())
    assert {c["M"] for c in cases} == set(R.SET_MS) and {c["V"] for c in cases} == set(R.SET_VS)
    assert {c["ngram"] for c in cases} == set(R.SET_NGRAMS) and {1, 2, 40, 448} <= {c["t"] for c in cases}
    assert any(c["bits_ld"] > R.words(c["V"]) for c in cases) and any(not c["has_static"] for c in cases)
    for c in cases:
        t, V = c["t"], c["V"]
        assert c["prefix"].shape == (c["M"], c["ld"]) and c["ld"] > t
        assert ((c["prefix"][:, t:] >= 0) & (c["prefix"][:, t:] < V)).all(), "a column past t must hold a token in range"
        longer = R.build_sets(c["prefix"], t + 1, V, R.set_case_static(c), c["ngram"])
        assert not np.array_equal(longer[0], R.set_case_expected(c)[0]), "reading column t would go unnoticed"
    bad = [c for c in cases if c["M"] >= 5 and c["t"] >= 6]
    assert all(any(int(v) in (-1, c["V"], 2 ** 31 - 1) for v in c["prefix"][1, :c["t"]]) for c in bad)


def test_head_cases_cover_what_they_claim():
    for d, V in itertools.product(R.HEAD_DS, R.HEAD_VS):
        pats = set()
        for M in R.HEAD_MS:
            c = R.head_case(d, V, M)
            pats |= set(c["patterns"])
            z = c["z"]
            assert np.abs(z * 8 - np.round(z * 8)).max() == 0 and np.abs(z).max() < 256
            for r, pat in enumerate(c["patterns"]):
                zp = R.constrain(z[r:r + 1], c["seen"][r:r + 1], c["banned"][r:r + 1], 2.0)[0]
                win, new = int(np.argsort(-z[r], kind="stable")[0]), int(np.argsort(-zp, kind="stable")[0])
                if pat == 0:
                    assert np.isneginf(zp[win]) and new // 128 != win // 128
                if pat == 1:
                    assert z[r, win] > 0 and zp[win] == z[r, win] / 2
                if pat == 2 and np.isfinite(zp).any():
                    assert zp[np.isfinite(zp)].max() < 0
                if pat == 3:
                    assert zp[new] == 0 and R.to_bool(c["seen"][r], V)[new]
                if pat == 5:
                    assert np.isfinite(zp).sum() == 1
                if pat == 6:
                    assert not np.isfinite(zp).any()
        assert pats == set(range(8)), (d, V, pats)


def test_undecided_rows_stay_under_the_cap():
    """The exact-score and random inputs of tests/test_constrain_kernels_gpu.py, from the reference alone."""
    for d, V in itertools.product(R.HEAD_DS, R.HEAD_VS):
        for cfg in R.HEAD_SAMPLE:
            dec = np.concatenate([R.head_expected(d, V, M, p)["sample"][cfg][2] for M in R.HEAD_MS for p in R.HEAD_PENALTIES])
            assert R.cap_ok(dec), (d, V, cfg, int((~dec).sum()), len(dec))
    for case in R.RANDOM_CASES:
        e = R.random_expected(case)
        assert R.cap_ok(e["argmax"][1]) and R.cap_ok(e["topk"][3]), case
        for cfg, (_, _, dec, _) in e["sample"].items():
            assert R.cap_ok(dec), (case, cfg, int((~dec).sum()))


def test_repeated_ngram_helper():
    assert R.has_repeated_ngram([1, 2, 3, 1, 2], 2) and not R.has_repeated_ngram([1, 2, 3, 2, 1], 2)
    assert R.has_repeated_ngram([4, 4, 4], 2) and not R.has_repeated_ngram([4, 4], 2)
    ban = R.step_banned([9, 1, 2, 3, 1], 10, 2, suppress=[7], begin=[8], first=True)
    assert set(np.nonzero(ban)[0]) == {2, 7, 8}
    assert set(np.nonzero(R.step_banned([9, 1, 2, 3, 1], 10, 2, suppress=[7], begin=[8]))[0]) == {2, 7}


# ----------------------------------------------------------------------------- 4. the library binds the new entry points
def test_library_exports_the_constraint_entry_points():
    from tethys_speech_amd import _lib
    h = _lib.lib()
    for name in ("tmi_decode_constraints", "tmi_lm_head_argmax_c", "tmi_lm_head_topk_c", "tmi_lm_head_sample_c"):
        assert name in _lib.SIGNATURES and getattr(h, name) is not None
    n = len(_lib.SIGNATURES["tmi_lm_head_argmax"][1])
    assert len(_lib.SIGNATURES["tmi_lm_head_argmax_c"][1]) == n + 4
    assert len(_lib.SIGNATURES["tmi_lm_head_topk_c"][1]) == len(_lib.SIGNATURES["tmi_lm_head_topk"][1]) + 4
    assert len(_lib.SIGNATURES["tmi_lm_head_sample_c"][1]) == len(_lib.SIGNATURES["tmi_lm_head_sample"][1]) + 4
    assert h.tmi_abi_version() == _lib.ABI_VERSION == 31
