"""The timestamp grammar without a GPU: the reference of rules a - f by enumeration on tiny vocabularies (its two forms
against each other and against hand-written expectations), ``parse_timestamp_segments`` on hand-written rows,
``transcribe_long`` with a scripted ``generate``, the validator's refusals, and the conditions on the rule g inputs the GPU
tests use (no undecided row among the planted ones, at most 5 % in the random tier)."""
import itertools

import numpy as np
import pytest
import torch

import _constrain_ref as C
import _timestamp_ref as T


def _whisper():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import whisper
    return whisper


# ----------------------------------------------------------------------------- rules a - f
TINY = ((40, 19), (45, 21), (33, 30), (64, 32))  # (V, tb): tb not a multiple of 8 or 32; V inside the last partial word


def _allowed(g, V, tb, P=0, no_ts=None, eos=2, max_initial=3, max_ts=None, fast=False):
    no_ts = tb - 1 if no_ts is None else no_ts
    max_ts = V - tb - 2 if max_ts is None else max_ts
    row = [7] + [5] * P + list(g)
    fn = T.rule_bans_fast if fast else T.rule_bans
    return sorted(np.nonzero(~fn(row, len(row), P, V, tb, no_ts, eos, max_initial, max_ts))[0])


@pytest.mark.parametrize("V,tb", TINY)
@pytest.mark.parametrize("P", (0, 2))
def test_rules_by_hand(V, tb, P):
    top = V - 2  # tb + max_ts: the last id, V - 1, is past the window
    text = [c for c in range(tb) if c != tb - 1]  # every below column but the no-timestamps id
    stamps = lambda lo, hi: list(range(lo, hi + 1))  # noqa: E731
    kw = dict(V=V, tb=tb, P=P)
    # n = 0: only the timestamps up to the cap
    assert _allowed([], **kw) == stamps(tb, min(tb + 3, top))
    assert _allowed([], max_initial=-1, **kw) == stamps(tb, top)
    assert _allowed([], max_initial=0, **kw) == [tb]
    # n = 1: an opening timestamp (last, and pen because n < 2): text or EOS, no timestamp
    assert _allowed([tb + 1], **kw) == text
    # n = 1: text first (only with a prompt-free caller who skipped rule b): text, or any timestamp (tl does not exist)
    assert _allowed([4], **kw) == text + stamps(tb, top)
    # n = 2: text behind a timestamp: text, or a timestamp strictly later (f)
    assert _allowed([tb + 1, 4], **kw) == text + stamps(tb + 2, top)
    # n = 2: two timestamps (a pair): text only (c)
    assert _allowed([tb + 1, tb + 2], **kw) == text
    # a closing timestamp: EOS, or a timestamp at or after it (d, e)
    assert _allowed([tb + 1, 4, tb + 2], **kw) == [2] + stamps(tb + 2, top)
    assert _allowed([tb + 1, 4, tb + 2], eos=-1, **kw) == stamps(tb + 2, top)
    # ... behind it the pair is complete: text only
    assert _allowed([tb + 1, 4, tb + 2, tb + 2], **kw) == text
    # tl at tb + max_ts: closing leaves EOS and tl itself; behind text nothing but text
    assert _allowed([tb + 1, 4, top], **kw) == [2, top]
    assert _allowed([tb + 1, 4, top, top, 4], **kw) == text
    # an id outside [0, V) is no timestamp
    assert _allowed([tb + 1, V], **kw) == text + stamps(tb + 2, top)
    assert _allowed([tb + 1, -1], **kw) == text + stamps(tb + 2, top)
    # no no-timestamps id: the column stays
    assert _allowed([tb + 1], no_ts=-1, **kw) == list(range(tb))


@pytest.mark.parametrize("V,tb", TINY)
def test_the_two_forms_of_the_reference_agree(V, tb):
    toks = [2, 4, tb - 1, tb, tb + 1, V - 2, V - 1, V, -1]
    for n in (0, 1, 2, 3):
        for g in itertools.product(toks, repeat=n):
            for P, mi, eos in ((0, 3, 2), (2, -1, -1)):
                a = _allowed(g, V, tb, P, max_initial=mi, eos=eos)
                assert a == _allowed(g, V, tb, P, max_initial=mi, eos=eos, fast=True), (g, P, mi, eos)


def test_apply_rules_only_adds_bits_below_V():
    V, tb = 45, 21
    W = C.words(V)
    prefix = np.array([[7, tb + 1, 4, tb + 2], [7, tb + 1, 4, 5]], dtype=np.int32)
    banned = np.zeros((2, W + 1), np.uint32)
    banned[:, W] = T.SENTINEL
    banned[0, 0] = 1 << 2  # EOS banned by the caller stays banned through rule d
    out = T.apply_rules(prefix, 4, 0, V, tb, tb - 1, 2, 3, V - tb - 2, banned)
    assert (out[:, W] == T.SENTINEL).all() and not (out[:, W - 1] >> (V & 31)).any()
    assert C.to_bool(out[0], V)[2] and (out & banned == banned).all()


def test_rule_cases_cover_the_states():
    for (V, tb), M, P in itertools.product(T.RULE_SHAPES, T.RULE_MS, T.RULE_PS):
        for c in T.rule_case(M, V, tb, P):
            e = T.rule_expected(c)
            assert e.shape == c["banned"].shape and (e[:, c["W"]] == T.SENTINEL).all()
            assert (e & c["banned"] == c["banned"]).all()
    names = set(n for c in T.rule_case(17, 200, 137, 0) for n in c["names"])
    assert {"n0", "n1", "open", "closing", "pair", "closing_top", "pair_top", "invalid_last"} <= names


# ----------------------------------------------------------------------------- parse_timestamp_segments
def test_parse_segments_by_hand():
    parse = _whisper().parse_timestamp_segments
    tb, W = 100, 1500
    t = lambda u: tb + u  # noqa: E731
    # pairs: two closed segments, then unfinished text -> advance to the last closed segment's end
    g = [t(0), 5, 6, t(50), t(50), 7, t(120), t(120), 8, 9]
    segs, adv = parse(g, tb, W)
    assert segs == [{"start": 0, "end": 50, "tokens": [5, 6]}, {"start": 50, "end": 120, "tokens": [7]}] and adv == 120
    # a single ending behind pairs: the tail is a segment too, and the whole window is consumed
    g = [t(0), 5, t(50), t(50), 7, t(130)]
    segs, adv = parse(g, tb, W)
    assert segs == [{"start": 0, "end": 50, "tokens": [5]}, {"start": 50, "end": 130, "tokens": [7]}] and adv == W
    # a pair at the very end is no single ending
    segs, adv = parse([t(10), 5, t(60), t(60)], tb, W)
    assert segs == [{"start": 10, "end": 60, "tokens": [5]}] and adv == 60
    # no pair, one closing timestamp: one segment from 0 to it
    segs, adv = parse([t(4), 5, 6, t(90)], tb, W)
    assert segs == [{"start": 0, "end": 90, "tokens": [5, 6]}] and adv == W
    # no timestamps at all, and nothing at all
    assert parse([5, 6], tb, W) == ([{"start": 0, "end": W, "tokens": [5, 6]}], W)
    assert parse([], tb, 700) == ([{"start": 0, "end": 700, "tokens": []}], 700)
    # only tb: the duration is the window's
    assert parse([t(0), 5], tb, W) == ([{"start": 0, "end": W, "tokens": [5]}], W)
    # EOS mid-row: everything from it on is cut, also timestamps behind it
    g = [t(0), 5, t(50), t(50), 7, 2, t(200), t(200), 9]
    segs, adv = parse(g, tb, W, eos_id=2)
    assert segs == [{"start": 0, "end": 50, "tokens": [5]}] and adv == 50
    assert parse(g, tb, W)[1] == 200  # (without an EOS id nothing is cut)
    assert parse(np.asarray(g, dtype=np.int32), tb, W, eos_id=2) == (segs, adv)


# ----------------------------------------------------------------------------- transcribe_long with a scripted generate
class _Cfg:
    vocab_size, eos_token_id, max_target_positions, n_mels = 1601, 2, 16, 4


class _FE:
    n_fft, hop = 400, 160

    def num_frames(self, n):
        return 1 + (n - self.n_fft) // self.hop if n >= self.n_fft else 0

    def __call__(self, wav):
        return torch.zeros(1, 4, self.num_frames(wav.numel())) + float(wav[0])


class _Scripted:
    """A model whose ``generate`` plays back rows and records what it was asked."""
    device, config = torch.device("cpu"), _Cfg()

    def __init__(self, rows):
        self.rows, self.calls, self._frontend = list(rows), [], _FE()

    def generate(self, feats, **kw):
        self.calls.append(dict(kw, frames=feats.shape[2], first=float(feats[0, 0, 0])))
        prompt = list(kw.get("prompt_ids", []))
        g = self.rows.pop(0)
        seq = torch.tensor([[50] + prompt + g], dtype=torch.int32)
        return {"sequences": seq, "lengths": torch.tensor([len(prompt) + len(g)], dtype=torch.int32)}


def test_transcribe_long_seeks_offsets_and_prompts():
    whisper = _whisper()
    tb = 100
    t = lambda u: tb + u  # noqa: E731
    n = 320000 + 480000 + 200000  # 62.5 s
    wav = np.arange(n, dtype=np.float32)
    rows = [
        [t(0), 5, 6, t(500), t(500), 7, t(1000), t(1000), 8, 2],        # closes at 20.00 s: seek 320000
        [t(10), 9, t(600), 2],                                           # single ending: the whole 1499-unit window
        [t(0), 11, 12, 2],                                               # the last, partial window; no closing timestamp
    ]
    model = _Scripted(rows)
    out = whisper.transcribe_long(model, wav, max_length=12, num_beams=2, repetition_penalty=1.1, prompt_ids=[3, 4])
    assert out["n_windows"] == 3 and not model.rows
    c0, c1, c2 = model.calls
    # seeks: 0, 1000 units * 320, + 1499 units * 320; the window is wav[seek : seek + 480000]
    assert [c["first"] for c in model.calls] == [0.0, 320000.0, 320000.0 + 1499 * 320]
    assert c0["frames"] == 2998 and c1["frames"] == 2998
    left = n - (320000 + 1499 * 320)
    assert c2["frames"] == 1 + (left - 400) // 160
    # prompts: the caller's while there is no text, then the text so far (timestamps are not text)
    assert c0["prompt_ids"] == [3, 4] and c1["prompt_ids"] == [5, 6, 7] and c2["prompt_ids"] == [5, 6, 7, 9]
    assert all(c["segment_timestamps"] is True and c["return_dict_in_generate"] and c["num_beams"] == 2 and
               c["repetition_penalty"] == 1.1 and c["max_initial_timestamp"] == 1.0 for c in model.calls)
    assert c0["max_length"] == 12 and c2["max_length"] == 12
    s = out["segments"]
    assert [x["ids"] for x in s] == [[5, 6], [7], [9], [11, 12]] and out["ids"] == [5, 6, 7, 9, 11, 12]
    assert [round(x["start"], 2) for x in s] == [0.0, 10.0, 20.0, round(20.0 + 29.98, 2)]
    units2 = (c2["frames"] + 1) // 2
    assert [round(x["end"], 2) for x in s] == [10.0, 20.0, 32.0, round(49.98 + units2 * 0.02, 2)]
    # the prompt keeps the last max_target_positions // 2 - 1 = 7 text tokens, and max_length shrinks to fit
    model = _Scripted([[t(0)] + list(range(20, 30)) + [t(700), t(700), 2], [t(0), 5, 2]])
    out = whisper.transcribe_long(model, wav[:480000 + 1000], max_length=12)
    assert "prompt_ids" not in model.calls[0] and model.calls[1]["prompt_ids"] == list(range(23, 30))
    assert model.calls[1]["max_length"] == 16 - 7 and model.calls[1]["first"] == 700 * 320.0
    # without conditioning every window gets the caller's prompt (here: none)
    model = _Scripted([[t(0), 5, t(700), t(700), 2], [t(0), 6, 2]])
    whisper.transcribe_long(model, wav[:480000 + 1000], condition_on_previous_text=False)
    assert all("prompt_ids" not in c for c in model.calls)
    # a tokenizer turns a segment's ids into text
    class Tok:
        def decode(self, ids):
            return "-".join(str(i) for i in ids)
    model = _Scripted([[t(0), 5, 6, 2]])
    out = whisper.transcribe_long(model, wav[:16000], tokenizer=Tok())
    assert out["segments"] == [{"start": 0.0, "end": 49 * 0.02, "text": "5-6"}] and model.calls[0]["frames"] == 98
    with pytest.raises(ValueError):
        whisper.transcribe_long(_Scripted([]), np.zeros((2, 16000), np.float32))
    with pytest.raises(AssertionError):  # a row that would not advance
        whisper.transcribe_long(_Scripted([[t(0), t(0), 5, 2]]), wav[:16000])


# ----------------------------------------------------------------------------- the validator
def test_validator_refusals_and_defaults():
    whisper = _whisper()
    cfg = whisper.make_config("small")
    chk = whisper.check_timestamp_rule_args
    assert chk(cfg) is None and chk(cfg, False, max_initial_timestamp=-5, timestamp_begin=-1) is None
    assert chk(cfg, True) == {"tb": 50364, "no_ts": 50363, "max_initial": 50}
    assert chk(cfg, True, None, 50000, -1) == {"tb": 50000, "no_ts": -1, "max_initial": -1}
    assert chk(cfg, True, 0.0)["max_initial"] == 0 and chk(cfg, True, min_length=0) is not None
    bad = [dict(timestamp_begin=0), dict(timestamp_begin=cfg.vocab_size), dict(timestamp_begin=1.5),
           dict(no_timestamps_token_id=50364), dict(no_timestamps_token_id=-2), dict(max_initial_timestamp=-0.1),
           dict(max_initial_timestamp=float("nan")), dict(eos_token_id=50364), dict(min_length=1),
           dict(suppress_tokens=[5, 50364]), dict(suppress_tokens=[cfg.vocab_size - 1]),
           dict(timestamp_begin=3, suppress_tokens=[0, 1]), dict(timestamp_begin=3, no_timestamps_token_id=-1, suppress_tokens=[0, 1, 2])]
    for kw in bad:
        with pytest.raises(ValueError):
            chk(cfg, True, **kw)
    assert chk(cfg, True, timestamp_begin=3, no_timestamps_token_id=-1, suppress_tokens=[0, 1]) is not None
    small = whisper.make_config("small", vocab_size=1000)
    with pytest.raises(ValueError):  # vocab_size - 1501 < 1
        chk(small, True)
    assert chk(small, True, timestamp_begin=900)["no_ts"] == 899
    with pytest.raises(ValueError):
        chk(whisper.make_config("small", vocab_size=70000), True)


def test_header_binding_and_abi_version():
    from tethys_speech_amd import _lib
    assert _lib.ABI_VERSION == 31
    for name in ("tmi_timestamp_rules", "tmi_lm_head_timestamp_gate", "tmi_lm_head_timestamp_gate_workspace_bytes"):
        assert name in _lib.SIGNATURES
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tethys_mi.h")).read()
    assert "int tmi_timestamp_rules(" in header and "int tmi_lm_head_timestamp_gate(" in header


# ----------------------------------------------------------------------------- conditions on the rule g inputs
def test_planted_inputs_are_all_decided_and_cover_both_outcomes():
    for (V, tb), Ms in ((T.GATE_SMALL, T.GATE_MS), (T.GATE_LARGE, (8,))):
        for M in Ms:
            c = T.planted_case(M, V, tb)
            assert c["decided"].all(), (M, V, c["names"], c["decided"])
            want = {"fire_single": True, "no_fire": False, "spread": True, "ts_banned": False, "below_banned": True,
                    "penalty_fires": True, "all_banned": False}
            for r, name in enumerate(c["names"]):
                if name in want:
                    assert bool(c["fired"][r]) == want[name], (M, V, r, name)
                if name == "spread":  # the LSE decides it, not a max
                    assert c["zp"][r, tb:].max() < c["below"][r] < c["lse"][r]
                if name == "penalty_fires":  # without the penalty it would not fire
                    assert not T.gate_ref(C.constrain(c["z"], None, c["banned"], 1.0), tb)[0][r]
                if name == "ts_banned":  # the bans decide it
                    assert T.gate_ref(c["z"], tb)[0][r]


def test_random_tier_is_mostly_decided_and_mixed():
    for case in T.RANDOM_CASES:
        c = T.random_case(*case)
        assert C.cap_ok(c["decided"], T.RANDOM_CAP), (case, int((~c["decided"]).sum()))
        assert c["fired"].any() and not c["fired"].all(), case
