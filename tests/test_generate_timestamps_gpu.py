"""``generate(segment_timestamps=True)`` and ``transcribe_long`` on the GPU: in every mode each returned row obeys the
timestamp grammar (rules a - f recomputed from the row by tests/_timestamp_ref.py), the teacher-forced fp64 replay of every
step agrees with the emitted token wherever rule g and the choice are decided, "segments" is ``parse_timestamp_segments``
of the row, and with ``segment_timestamps=None`` the call is the call it was.  The reduced model, oracle parameters and
features are tests/test_generate_gpu.py's ``_setup``: 402 feature frames are 201 encoder frames, so the largest timestamp
is tb + 201 and rule a's cap is at work."""
import numpy as np
import pytest
import torch

import _timestamp_ref as T
from test_generate_gpu import _mods, _model, _oracle_prefix_logits, _setup

pytestmark = pytest.mark.gpu

V, TB, NO_TS, EOS = 51865, 50364, 50363, 2
T_IN, MAX_TS, L = 402, 201, 12
MAX_INITIAL = 50  # 1.0 s
MODES = (("greedy", dict()), ("beam", dict(num_beams=3, num_return_sequences=3)),
         ("sample", dict(do_sample=True, top_k=8, seed=5, temperature=0.9)))


def _rows(out, P=0):
    seq = out["sequences"].cpu().numpy()
    lens = out["lengths"].cpu().numpy() if "lengths" in out else np.full(seq.shape[0], seq.shape[1] - 1)
    return seq, lens


def _check_rows(whisper, out, eos, P=0, prompt=()):
    seq, lens = _rows(out)
    assert len(out["segments"]) == seq.shape[0] and len(out["advance"]) == seq.shape[0]
    for r in range(seq.shape[0]):
        assert list(seq[r, 1:1 + P]) == list(prompt)
        g = [int(v) for v in seq[r, 1 + P:1 + int(lens[r])]]
        bad = T.grammar_ok(g, V, TB, NO_TS, eos, MAX_INITIAL, MAX_TS)
        assert bad < 0, ("a token the grammar bans", r, bad, g)
        assert g and g[0] >= TB and g[0] <= TB + MAX_INITIAL and NO_TS not in g and max(g) <= TB + MAX_TS, (r, g)
        segs, adv = whisper.parse_timestamp_segments(g, TB, MAX_TS, eos)
        assert out["segments"][r] == segs and out["advance"][r] == adv and adv > 0, (r, g, out["segments"][r])
        for s in segs:
            assert 0 <= s["start"] <= s["end"] <= MAX_TS and all(x < TB for x in s["tokens"])


def _replay(O, params, ocfg, enc, seq, lens, rows_per_item, eos, rel, exact_choice, P=0):
    """Teacher-forced fp64 replay: at every generated position of every row, rules a - g on the oracle's logits of the row's
    own prefix; where rule g is decided (|lse_ts - max_below| > rel * max|z|, the bound tests/test_generate_constrained_gpu.py
    uses for this model's logits) a fired row's token is a timestamp, and with ``exact_choice`` (greedy) the token is the
    argmax of z' where its lead is clear too.  -> (decided fired, decided not fired) counts."""
    n_fired = n_quiet = 0
    ids = torch.from_numpy(seq.astype(np.int64))
    enc_rows = enc.repeat_interleave(rows_per_item, dim=0)
    for t in range(1 + P, seq.shape[1]):
        live = [r for r in range(seq.shape[0]) if t <= int(lens[r]) and (eos < 0 or eos not in seq[r, 1 + P:t].tolist())]
        if not live:
            continue
        z = _oracle_prefix_logits(O, params, ocfg, enc_rows[live], ids[live], t).numpy()
        for i, r in enumerate(live):
            b = rel * (np.abs(z[i]).max() + 1e-6)
            ban, zp, fired, decided = T.step_ref(seq[r], t, P, z[i], V, TB, NO_TS, eos, MAX_INITIAL, MAX_TS, b=b / 2)
            tok = int(seq[r, t])
            if not decided:
                continue
            n_fired, n_quiet = n_fired + fired, n_quiet + (not fired)
            if fired:
                assert tok >= TB, ("rule g fired in the replay, the token is no timestamp", r, t, tok)
            assert not ban[tok], ("a banned token", r, t, tok)
            if exact_choice:
                top2 = np.sort(zp)[-2:]
                if top2[1] - top2[0] > b:
                    assert tok == int(np.argmax(zp)), (r, t, tok, int(np.argmax(zp)))
    return n_fired, n_quiet


@pytest.mark.parametrize("name,mode", MODES, ids=[m[0] for m in MODES])
def test_rows_obey_the_grammar_and_follow_the_replay(dev, name, mode):
    _, whisper, O = _mods()
    ocfg, params, feats, enc = _setup(T_IN)
    f = feats.to(dev)
    R = mode.get("num_return_sequences", 1)
    fired_total = 0
    for precision, rel in (("fp32", 1e-4), ("bf16", 5e-2)):
        model = _model(dev, precision, params)
        for eos in (EOS, -1):
            out = model.generate(f, max_length=L, segment_timestamps=True, eos_token_id=eos, **mode)
            assert isinstance(out, dict) and {"sequences", "segments", "advance"} <= set(out)
            _check_rows(whisper, out, eos)
            seq, lens = _rows(out)
            nf, nq = _replay(O, params, ocfg, enc, seq, lens, R, eos, rel, exact_choice=name == "greedy" and precision == "fp32")
            fired_total += nf
            again = model.generate(f, max_length=L, segment_timestamps=True, eos_token_id=eos, **mode)
            assert torch.equal(again["sequences"], out["sequences"]) and again["segments"] == out["segments"]
    assert fired_total > 0, "rule g never fired in a decided step: the replay checked nothing of it"


def test_prompt_constraints_and_token_timestamps_combine(dev):
    _, whisper, _ = _mods()
    _, params, feats, _ = _setup(T_IN)
    model = _model(dev, "bf16", params)
    f = feats.to(dev)
    prompt = [11, 22, 33]
    for _, mode in MODES:
        out = model.generate(f, max_length=8, segment_timestamps=True, prompt_ids=prompt, no_repeat_ngram_size=2,
                             repetition_penalty=1.2, suppress_tokens=[7, 8], max_initial_timestamp=1.0, **mode)
        _check_rows(whisper, out, EOS, P=3, prompt=prompt)
        seq, lens = _rows(out)
        assert not (set(seq[:, 4:].reshape(-1).tolist()) & {7, 8})
    out = model.generate(f, max_length=6, segment_timestamps=True, return_token_timestamps=True)
    assert {"segments", "advance", "token_start_times", "token_end_times"} <= set(out)
    _check_rows(whisper, out, EOS)
    # max_initial_timestamp: 0 pins the first token to <|0.00|>, None lifts the cap
    first = model.generate(f, max_length=1, segment_timestamps=True, max_initial_timestamp=0.0)["sequences"][:, 1]
    assert first.cpu().tolist() == [TB] * f.shape[0]
    free = model.generate(f, max_length=1, segment_timestamps=True, max_initial_timestamp=None)["sequences"][:, 1].cpu()
    assert bool(((free >= TB) & (free <= TB + MAX_TS)).all())
    with pytest.raises(ValueError):
        model.generate(f, max_length=4, segment_timestamps=True, do_sample=True, min_length=2)
    with pytest.raises(ValueError):
        model.generate(f, max_length=4, segment_timestamps=True, suppress_tokens=[TB + 5])


def _counting(ops, monkeypatch):
    calls = {}
    for name in dir(ops):
        fn = getattr(ops, name)
        if name in ("dt", "ptr", "stream", "set_stream", "constraint_words"):
            continue
        if callable(fn) and getattr(fn, "__module__", None) == ops.__name__ and not isinstance(fn, type) and not name.startswith("_"):
            def wrap(*a, _fn=fn, _name=name, **k):
                calls[_name] = calls.get(_name, 0) + 1
                return _fn(*a, **k)
            monkeypatch.setattr(ops, name, wrap)
    return calls


def test_off_is_the_call_it_was(dev, monkeypatch):
    """``segment_timestamps`` None or False, whatever the other three arguments hold: the same results bit for bit and the
    same calls into ``ops`` as without the arguments, alone and beside an n-gram ban; True adds exactly one
    tmi_timestamp_rules and one gate launch per step behind the set builder and swaps the head for its _c form."""
    ops, whisper, _ = _mods()
    _, params, feats, _ = _setup(T_IN)
    model = _model(dev, "bf16", params)
    f = feats.to(dev)
    calls = _counting(ops, monkeypatch)
    new = {"timestamp_rules", "lm_head_timestamp_gate", "lm_head_timestamp_gate_workspace_elems"}
    off = dict(max_initial_timestamp=0.5, timestamp_begin=123, no_timestamps_token_id=5)
    for mode in (dict(), dict(num_beams=3, return_dict_in_generate=True),
                 dict(do_sample=True, top_k=8, seed=3, return_dict_in_generate=True)):
        head = "lm_head_sample" if "do_sample" in mode else "lm_head_topk" if "num_beams" in mode else "lm_head_argmax"
        for extra in (dict(), dict(no_repeat_ngram_size=2)):
            model.generate(f, max_length=6, eos_token_id=-1, **mode, **extra)  # (the mode's buffers exist from here on)
            calls.clear()
            a = model.generate(f, max_length=6, eos_token_id=-1, **mode, **extra)
            seen_a = dict(calls)
            for flag in (None, False):
                calls.clear()
                b = model.generate(f, max_length=6, eos_token_id=-1, segment_timestamps=flag, **off, **mode, **extra)
                if isinstance(a, dict):
                    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
                else:
                    assert torch.equal(a, b)
                assert dict(calls) == seen_a and not new & set(calls), (mode, extra, flag, seen_a, dict(calls))
        calls.clear()
        model.generate(f, max_length=6, eos_token_id=-1, **mode)
        plain = dict(calls)
        calls.clear()
        model.generate(f, max_length=6, eos_token_id=-1, segment_timestamps=True, **mode)
        assert calls["timestamp_rules"] == 6 and calls["lm_head_timestamp_gate"] == 6 and calls["decode_constraints"] == 6
        assert calls[head + "_c"] == 6 and head not in calls
        added = new | {"decode_constraints", head + "_c"}
        assert {k: v for k, v in calls.items() if k not in added} == {k: v for k, v in plain.items() if k != head}


def test_transcribe_long_walks_seventy_seconds(dev):
    """70 s of seeded noise through the reduced model: at least the three windows a walk in whole windows takes, segment
    times inside the audio and in order within and across windows, text ids only in the segments, every window's first
    call conditioned on the text so far."""
    _, whisper, _ = _mods()
    _, params, _, _ = _setup(T_IN)
    model = _model(dev, "bf16", params)
    wav = np.random.RandomState(3).randn(16000 * 70).astype(np.float32)
    out = whisper.transcribe_long(model, wav, max_length=10)
    assert out["n_windows"] >= 3, out["n_windows"]
    segs = out["segments"]
    assert segs and all(0.0 <= s["start"] <= s["end"] <= 70.0 + 1e-6 for s in segs)
    starts = [s["start"] for s in segs]
    assert all(a <= b + 1e-9 for a, b in zip(starts[:-1], starts[1:])), starts
    ends = [s["end"] for s in segs]
    assert all(a <= b + 1e-9 for a, b in zip(ends[:-1], ends[1:])), ends
    assert all(x < TB for s in segs for x in s["ids"]) and out["ids"] == [x for s in segs for x in s["ids"]]
    again = whisper.transcribe_long(model, wav, max_length=10)
    assert again == out
