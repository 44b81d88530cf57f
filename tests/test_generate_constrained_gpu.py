"""``generate`` with decode constraints and prompts on the GPU: greedy under no_repeat_ngram_size and a prompt against the
fp64 oracle loop under the same rule, the invariants of beam search and sampling, repetition_penalty against the
reference's choice, the defaults' unchanged path (results and the calls seen through ``ops``), token timestamps over a
prompt, ``transcribe_audio`` and the command line.  The reduced model, oracle parameters and features are
tests/test_generate_gpu.py's ``_setup``; the feature seed 402 was picked on the CPU: the UNCONSTRAINED oracle transcript
of both rows repeats a bigram within 24 steps (asserted below before anything is launched)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import _constrain_ref as R
from _margins import within
from test_generate_gpu import _mods, _model, _oracle_prefix_logits, _setup

pytestmark = pytest.mark.gpu

V = 51865
T_IN, L = 402, 24
START = 50257


def _oracle_loop(O, params, ocfg, enc, B, steps, prompt=None, ngram=0):
    """Greedy decoding in fp64 under the rule: -> ids [B, 1 + P + steps] (no EOS stop)."""
    ids = torch.full((B, 1), START, dtype=torch.int64)
    if prompt is not None:
        ids = torch.cat([ids, torch.as_tensor(prompt, dtype=torch.int64).reshape(1, -1).expand(B, -1)], 1)
    for _ in range(steps):
        z = _oracle_prefix_logits(O, params, ocfg, enc, ids, ids.shape[1])
        for b in range(B):
            z[b, torch.from_numpy(R.step_banned(ids[b].tolist(), V, ngram))] = -np.inf
        ids = torch.cat([ids, z.argmax(1)[:, None]], 1)
    return ids


def _rows_ok(rows, lengths, P, suppress, begin, ngram, prompt):
    """The invariants of one result: rows [N, 1 + n] (numpy), lengths [N] counting prompt plus generated tokens."""
    for row, n in zip(rows, lengths):
        toks = [int(v) for v in row[:1 + n]]
        assert toks[0] == START and toks[1:1 + P] == list(prompt), ("the prompt is not echoed", toks)
        gen = toks[1 + P:]
        assert not set(gen) & set(suppress), ("a suppressed token", toks)
        assert not gen or gen[0] not in begin, ("a begin-suppressed token first", toks)
        assert not ngram or not R.has_repeated_ngram(toks, ngram), ("an n-gram twice", toks)


def test_greedy_no_repeat_bigram_follows_the_oracle(dev):
    _, whisper, O = _mods()
    ocfg, params, feats, enc = _setup(T_IN)
    B = feats.shape[0]
    free = _oracle_loop(O, params, ocfg, enc, B, L)
    assert all(R.has_repeated_ngram(free[b].tolist(), 2) for b in range(B)), "the seed no longer shows a repeated bigram"
    for prompt in (None, [33348, 7]):
        P = 0 if prompt is None else len(prompt)
        ref = _oracle_loop(O, params, ocfg, enc, B, L, prompt, ngram=2)
        assert not any(R.has_repeated_ngram(ref[b].tolist(), 2) for b in range(B))
        for precision, rel in (("fp32", 1e-4), ("bf16", 5e-2)):
            model = _model(dev, precision, params)
            ids = model.generate(feats.to(dev), max_length=L, no_repeat_ngram_size=2, prompt_ids=prompt, eos_token_id=-1)
            assert ids.dtype == torch.int32 and tuple(ids.shape) == (B, 1 + P + L)
            ids = ids.cpu().long()
            _rows_ok(ids.numpy(), [P + L] * B, P, (), (), 2, prompt or [])
            all_clear = True
            for t in range(1 + P, ids.shape[1]):
                z = _oracle_prefix_logits(O, params, ocfg, enc, ids, t)  # teacher-forced on the model's own prefix
                scale = z.abs().max(1).values + 1e-6
                for b in range(B):
                    z[b, torch.from_numpy(R.step_banned(ids[b, :t].tolist(), V, 2))] = -np.inf
                top2 = z.topk(2, dim=1)
                clear = (top2.values[:, 0] - top2.values[:, 1]) > rel * scale
                all_clear &= bool(clear.all())
                if precision == "fp32":
                    assert torch.equal(ids[clear, t], top2.indices[clear, 0]), (t, ids[:, t], top2.indices[:, 0])
                chosen = z.gather(1, ids[:, t:t + 1])[:, 0]
                within(f"generate no_repeat_ngram {precision} (max z' - chosen z') / max|z|",
                       float(((top2.values[:, 0] - chosen) / scale).max()), rel)
            if precision == "fp32" and all_clear:
                assert torch.equal(ids, ref), (ids, ref)
            again = model.generate(feats.to(dev), max_length=L, no_repeat_ngram_size=2, prompt_ids=prompt, eos_token_id=-1)
            assert torch.equal(again.cpu().long(), ids)


def test_beam_and_sampling_invariants(dev):
    _, whisper, _ = _mods()
    _, params, feats, _ = _setup(T_IN)
    B, K, Rr, P, steps = feats.shape[0], 3, 3, 3, 12
    f = feats.to(dev)
    model = _model(dev, "bf16", params)
    prompt = [11, 22, 33]
    # suppress what the unconstrained run emits most, begin-suppress what then comes first: both lists matter
    plain = model.generate(f, max_length=steps, prompt_ids=prompt, eos_token_id=-1)[:, 1 + P:].cpu().numpy()
    vals, counts = np.unique(plain, return_counts=True)
    suppress = [int(v) for v in vals[np.argsort(-counts)][:2]] + [0]
    first = model.generate(f, max_length=1, prompt_ids=prompt, suppress_tokens=suppress)[:, 1 + P].cpu().tolist()
    begin = sorted(set(int(v) for v in first))
    kw = dict(max_length=steps, prompt_ids=prompt, suppress_tokens=suppress, begin_suppress_tokens=begin,
              no_repeat_ngram_size=2, repetition_penalty=1.2, return_dict_in_generate=True)
    # beam search
    out = model.generate(f, num_beams=K, num_return_sequences=Rr, **kw)
    seq, lens, scores = out["sequences"].cpu().numpy(), out["lengths"].cpu().numpy(), out["sequences_scores"].cpu().numpy()
    assert seq.shape[0] == B * Rr and lens.shape == (B * Rr,) and scores.shape == (B * Rr,)
    assert seq.shape[1] == 1 + lens.max() and (lens > P).all() and (lens <= P + steps).all() and np.isfinite(scores).all()
    assert (scores <= 0).all() and (scores.reshape(B, Rr)[:, :-1] >= scores.reshape(B, Rr)[:, 1:]).all()
    _rows_ok(seq, lens, P, suppress, begin, 2, prompt)
    # generated tokens only in the scores: one generated token, length_penalty 1 -> the score is that token's
    # log-probability, whatever the prompt's length (a score over prompt + 1 tokens would be divided by P + 1)
    one = model.generate(f, num_beams=K, max_length=1, prompt_ids=prompt, eos_token_id=-1, return_dict_in_generate=True)
    ref = model.score(f, one["sequences"], one["lengths"])
    lp_last = ref["token_logprobs"][:, P].cpu().numpy() if isinstance(ref, dict) else None
    assert (one["lengths"].cpu().numpy() == P + 1).all()
    if lp_last is not None:
        within("beam score of one generated token after a prompt vs score()", float(np.abs(one["sequences_scores"].cpu().numpy() - lp_last).max()), 5e-2)
    # sampling
    out = model.generate(f, do_sample=True, top_k=8, seed=5, min_length=2, **kw)
    seq, lens = out["sequences"].cpu().numpy(), out["lengths"].cpu().numpy()
    n = seq.shape[1] - 1 - P
    lp = out["token_logprobs"].cpu().numpy()
    assert seq.shape[0] == B and 1 <= n <= steps and lp.shape == (B, n) and (lens >= P + min(2, n)).all() and (lens <= P + n).all()
    assert np.isfinite(lp).all() and (lp <= 0).all()
    assert np.allclose(out["sequences_scores"].cpu().numpy(), lp.sum(1), atol=1e-4)
    _rows_ok(seq, lens, P, suppress, begin, 2, prompt)
    again = model.generate(f, do_sample=True, top_k=8, seed=5, min_length=2, **kw)
    assert all(torch.equal(out[k], again[k]) for k in out)
    other = model.generate(f, do_sample=True, top_k=8, seed=6, min_length=2, **kw)
    assert not torch.equal(other["sequences"], out["sequences"]) or n == 0
    # per-item prompts [B, P]
    per_item = np.array([[11, 22, 33], [44, 55, 66]])[:B]
    seq = model.generate(f, max_length=4, prompt_ids=per_item, no_repeat_ngram_size=1, eos_token_id=-1).cpu().numpy()
    assert np.array_equal(seq[:, 1:4], per_item) and all(len(set(r.tolist())) == len(r) for r in seq)
    with pytest.raises(ValueError):
        model.generate(f, max_length=4, prompt_ids=np.zeros((B + 1, 2), dtype=np.int64))


def test_repetition_penalty_changes_the_first_token_to_the_references(dev):
    _, whisper, O = _mods()
    ocfg, params, feats, enc = _setup(T_IN)
    B = feats.shape[0]
    model = _model(dev, "fp32", params)
    f = feats.to(dev)
    u = model.generate(f, max_length=1)[:, 1].cpu().long()      # the unconstrained first token of each row ...
    prompt = u[:, None].numpy()                                   # ... as the row's prompt
    plain = model.generate(f, max_length=1, prompt_ids=prompt, eos_token_id=-1).cpu().long()
    pen = model.generate(f, max_length=1, prompt_ids=prompt, repetition_penalty=1e6, eos_token_id=-1).cpu().long()
    assert tuple(pen.shape) == (B, 3) and torch.equal(pen[:, :2], plain[:, :2]) and torch.equal(pen[:, 1], u)
    z = _oracle_prefix_logits(O, params, ocfg, enc, plain, 2).numpy()
    seen = np.stack([R.bitset([START, int(u[b])], V) for b in range(B)])
    zp = R.constrain(z, seen, None, 1e6)
    scale = np.abs(z).max(1) + 1e-6
    tok, _ = R.argmax_ref(zp)
    top2 = -np.sort(-zp, axis=1)[:, :2]
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4 * scale
    assert clear.any(), "no decided row: the check would be empty"
    assert np.array_equal(pen[:, 2].numpy()[clear], tok[clear]), (pen[:, 2], tok)
    hit = np.isin(plain[:, 2].numpy(), [START]) | (plain[:, 2].numpy() == u.numpy())
    assert hit.any(), "the unpenalised token is not a seen one: the penalty would have nothing to change"
    assert (pen[:, 2].numpy()[hit & clear] != plain[:, 2].numpy()[hit & clear]).all()


def _counting(ops, monkeypatch):
    """Wrap every function of ``ops`` with a counter (the argument helpers dt / ptr / stream / constraint_words aside: they launch nothing):
    -> the dict name -> calls."""
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


def test_defaults_take_the_unconstrained_path(dev, monkeypatch):
    ops, whisper, _ = _mods()
    _, params, feats, _ = _setup(T_IN)
    model = _model(dev, "bf16", params)
    f = feats.to(dev)
    off = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, suppress_tokens=[], begin_suppress_tokens=[])
    calls = _counting(ops, monkeypatch)
    new = {"decode_constraints", "lm_head_argmax_c", "lm_head_topk_c", "lm_head_sample_c"}
    for mode in (dict(), dict(num_beams=3, return_dict_in_generate=True),
                 dict(do_sample=True, top_k=8, seed=3, return_dict_in_generate=True)):
        model.generate(f, max_length=6, eos_token_id=-1, **mode)  # (the mode's buffers exist from here on)
        calls.clear()
        a = model.generate(f, max_length=6, eos_token_id=-1, **mode)
        seen_a = dict(calls)
        calls.clear()
        b = model.generate(f, max_length=6, eos_token_id=-1, **mode, **off)
        seen_b = dict(calls)
        if isinstance(a, dict):
            assert all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)
        else:
            assert torch.equal(a, b)
        assert seen_a == seen_b and not new & set(seen_a), (mode, seen_a, seen_b)
        head = "lm_head_sample" if "do_sample" in mode else "lm_head_topk" if "num_beams" in mode else "lm_head_argmax"
        assert seen_a[head] == 6
        # ... and an active constraint swaps exactly the LM head for its _c form, plus one set-builder launch per step
        calls.clear()
        model.generate(f, max_length=6, eos_token_id=-1, no_repeat_ngram_size=2, **mode)
        assert calls[head + "_c"] == 6 and calls["decode_constraints"] == 6 and head not in calls
        assert {k: v for k, v in calls.items() if k not in new} == {k: v for k, v in seen_a.items() if k != head}
        # a prompt alone keeps the unconstrained head
        calls.clear()
        model.generate(f, max_length=6, eos_token_id=-1, prompt_ids=[5, 6], **mode)
        assert calls[head] == 6 and not new & set(calls)


def test_zero_and_one_step_forms_of_every_mode(dev, monkeypatch):
    """The forms that never enter, or barely enter, the step loop: ``max_length=0`` returns [start, prompt...] per row
    without one call into ``ops``, and one step behind a prompt of two appends one column and leaves the prompt alone."""
    ops, whisper, _ = _mods()
    _, params, feats, _ = _setup(T_IN)
    model = _model(dev, "bf16", params)
    f = feats.to(dev)
    B = f.shape[0]
    calls = _counting(ops, monkeypatch)
    for mode, Rr, keys in ((dict(), 1, None),  # (the greedy path has no dict form: it returns the ids either way)
                           (dict(num_beams=2, num_return_sequences=2), 2, {"sequences", "sequences_scores", "lengths"}),
                           (dict(do_sample=True, top_k=8, seed=1), 1,
                            {"sequences", "token_logprobs", "sequences_scores", "lengths"})):
        for prompt in ([], [9, 8]):
            P, rows = len(prompt), B * Rr
            want = torch.tensor([[START] + prompt] * rows, dtype=torch.int32)
            calls.clear()
            ids = model.generate(f, max_length=0, prompt_ids=prompt or None, **mode)
            out = model.generate(f, max_length=0, prompt_ids=prompt or None, return_dict_in_generate=True, **mode)
            assert not calls, (mode, prompt, calls)
            assert ids.dtype == torch.int32 and torch.equal(ids.cpu(), want), (mode, prompt, ids)
            if keys is None:
                assert torch.equal(out.cpu(), want)
                continue
            assert set(out) == keys and out["sequences"].dtype == torch.int32 and torch.equal(out["sequences"].cpu(), want)
            assert out["lengths"].dtype == torch.int32 and out["lengths"].cpu().tolist() == [P] * rows
            assert out["sequences_scores"].cpu().tolist() == [0.0] * rows
            if "token_logprobs" in keys:
                assert tuple(out["token_logprobs"].shape) == (B, 0)
        one = model.generate(f, max_length=1, prompt_ids=[9, 8], eos_token_id=-1, **mode)
        assert tuple(one.shape) == (B * Rr, 1 + 2 + 1) and torch.equal(one[:, :3].cpu(), want), (mode, one)


def test_token_timestamps_cover_prompt_and_transcript(dev):
    _, whisper, _ = _mods()
    _, params, feats, _ = _setup(T_IN)
    model = _model(dev, "bf16", params)
    f = feats.to(dev)
    B, P = f.shape[0], 2
    for mode in (dict(), dict(num_beams=2), dict(do_sample=True, top_k=8, seed=1)):
        out = model.generate(f, max_length=6, prompt_ids=[9, 8], no_repeat_ngram_size=2, return_token_timestamps=True, **mode)
        seq = out["sequences"]
        lens = out["lengths"].cpu().numpy() if "lengths" in out else np.full(B, seq.shape[1] - 1)
        t0, t1 = out["token_start_times"].cpu().numpy(), out["token_end_times"].cpu().numpy()
        assert t0.shape == (B, seq.shape[1] - 1) and t1.shape == t0.shape and (lens > P).all()
        for b in range(B):
            n = int(lens[b])
            assert np.isfinite(t0[b, :n]).all() and (t0[b, :n] <= t1[b, :n]).all() and (np.diff(t0[b, :n]) >= 0).all()
        assert np.array_equal(seq[:, 1:1 + P].cpu().numpy(), np.tile([9, 8], (B, 1)))
    with pytest.raises(ValueError):  # one position less with timestamps
        model.generate(f, max_length=447, prompt_ids=[9], return_token_timestamps=True)


def test_transcribe_audio_and_the_command_line(dev, capsys):
    _, whisper, _ = _mods()
    _, params, _, _ = _setup(T_IN)
    model = _model(dev, "bf16", params)
    got = whisper.transcribe_audio(model, None, max_length=8, no_repeat_ngram_size=2, prompt_ids=[7, 8])
    assert isinstance(got, np.ndarray) and got[0] == START and list(got[1:3]) == [7, 8] and 4 <= len(got) <= 11
    assert not R.has_repeated_ngram(got.tolist(), 2)
    res = whisper.transcribe_audio(model, None, max_length=8, no_repeat_ngram_size=2, prompt_ids=[7, 8], num_beams=2,
                                   suppress_tokens=[int(got[3])], return_timestamps=True)
    assert list(res["ids"][1:3]) == [7, 8] and int(got[3]) not in res["ids"][3:].tolist()
    assert len(res["token_start_times"]) == len(res["ids"]) - 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("whisper_transcribe", os.path.join(root, "speech_jobs", "whisper_transcribe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    capsys.readouterr()
    mod.main(["--model_type", "tiny", "--max_length", "6", "--repetition_penalty", "1.3", "--no_repeat_ngram_size", "2",
              "--suppress_tokens", "1,2,3", "--begin_suppress_tokens", "4,5", "--prompt_ids", "10,11"])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    ids = lines[0]["ids"]
    assert ids[:3] == [START, 10, 11] and lines[0]["n_tokens"] == len(ids) - 1 and 4 <= len(ids) <= 9
    assert not set(ids[3:]) & {1, 2, 3} and ids[3] not in (4, 5) and not R.has_repeated_ngram(ids, 2)
    with pytest.raises(ValueError):
        mod.main(["--model_type", "tiny", "--max_length", "6", "--suppress_tokens", "99999"])
