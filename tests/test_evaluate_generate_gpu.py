"""``WhisperForConditionalGeneration.evaluate_generate``, ``train.evaluate_generate_whisper`` and ``whisper_eval.py --generate``
on the GPU, tiny configuration: the counts equal the reference of tests/_edit_ref.py applied on the host to the sequences,
lengths and labels of that same call.  Integers throughout: every comparison is an equality."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import _edit_ref as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TINY = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, vocab_size=160, encoder_layers=2,
             decoder_layers=2, n_mels=16, n_ctx=32, decoder_start_token_id=150, max_target_positions=32)
B, T_IN, S, EOS, TB = 3, 48, 9, 2, 120
MODES = (("greedy", dict()),
         ("beam", dict(num_beams=3, num_return_sequences=2)),
         ("sample", dict(do_sample=True, top_k=8, seed=5, temperature=0.9)),
         ("prompt", dict(prompt_ids=[11, 22, 33])),
         ("timestamps", dict(segment_timestamps=True, timestamp_begin=TB)),
         ("timestamps-beam", dict(segment_timestamps=True, timestamp_begin=TB, num_beams=3, num_return_sequences=3)))
COUNT_KEYS = ("n_edits", "n_sub", "n_del", "n_ins", "n_ref_tokens", "n_hyp_tokens", "n_exact", "n_items", "n_oracle_edits",
              "token_error_rate", "oracle_error_rate")


@pytest.fixture(scope="module")
def setup(dev):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import whisper
    model = whisper.create_whisper_model("small", device=dev, precision="bf16", seed=11, **_TINY)
    rng = np.random.default_rng(4)
    feats = torch.from_numpy(rng.standard_normal((B, 16, T_IN)).astype(np.float32)).to(dev)
    labels = rng.integers(3, 140, (B, S)).astype(np.int32)  # text ids and, from TB on, timestamp ids
    labels[0, 6] = EOS   # cut before it
    labels[1, 0] = TB + 3
    lens = np.asarray([S, 7, 4], np.int32)
    return model, feats, labels, lens


def _host(res, labels, lens, P, eos, skip):
    seq = res["sequences"].cpu().numpy()
    R = seq.shape[0] // labels.shape[0]
    hl = None if res["lengths"] is None else res["lengths"].cpu().numpy() - P
    want = E.reference(seq[:, 1 + P:], labels, hl, lens, R=R, stop_id=eos, skip=skip)
    return want, R


@pytest.mark.parametrize("name,mode", MODES, ids=[m[0] for m in MODES])
def test_counts_equal_the_reference_on_the_same_sequences(setup, name, mode):
    model, feats, labels, lens = setup
    for eos, ll in ((EOS, lens), (-1, None)):
        res = model.evaluate_generate(feats, torch.from_numpy(labels), None if ll is None else torch.from_numpy(ll),
                                      return_items=True, max_length=8, eos_token_id=eos, **mode)
        P = len(mode.get("prompt_ids", ()))
        skip = (TB, 160) if mode.get("segment_timestamps") else (0, 0)
        want, R = _host(res, labels, ll, P, eos, skip)
        assert R == mode.get("num_return_sequences", 1) and res["sequences"].shape[0] == B * R
        assert res["edits"].dtype == torch.int32 and np.array_equal(res["edits"].cpu().numpy(), want)
        ref = E.counts(want, R)
        assert {k: res[k] for k in COUNT_KEYS} == ref and all(isinstance(res[k], float) for k in COUNT_KEYS)
        assert res["n_oracle_edits"] == sum(min(int(want[b * R + k, 0]) for k in range(R)) for b in range(B))
        assert res["n_oracle_edits"] <= res["n_edits"] and (R > 1 or res["n_oracle_edits"] == res["n_edits"])
        if mode.get("segment_timestamps"):  # the hypothesis side held timestamps and lost them
            seq = res["sequences"].cpu().numpy()[:, 1:]
            assert (seq >= TB).any()
        plain = model.evaluate_generate(feats, torch.from_numpy(labels), None if ll is None else ll, max_length=8,
                                        eos_token_id=eos, **mode)
        assert plain == {k: res[k] for k in COUNT_KEYS}  # without return_items: the same numbers and nothing else


def test_labels_equal_to_the_generated_tokens_and_one_changed(setup):
    model, feats, _, _ = setup
    seq = model.generate(feats, max_length=8, eos_token_id=-1)
    labels = seq[:, 1:].contiguous()
    res = model.evaluate_generate(feats, labels, max_length=8, eos_token_id=-1)
    assert res["n_edits"] == 0.0 and res["token_error_rate"] == 0.0 and res["n_exact"] == float(B) and res["n_ref_tokens"] == 8.0 * B
    changed = labels.clone()
    changed[1, 3] = (changed[1, 3] + 1) % 100
    res = model.evaluate_generate(feats, changed, max_length=8, eos_token_id=-1)
    assert (res["n_edits"], res["n_sub"], res["n_del"], res["n_ins"], res["n_exact"]) == (1.0, 1.0, 0.0, 0.0, B - 1.0)
    # a reference one token shorter: the last generated token is an insertion
    res = model.evaluate_generate(feats, labels, torch.tensor([8, 7, 8]), max_length=8, eos_token_id=-1)
    assert (res["n_edits"], res["n_sub"], res["n_del"], res["n_ins"]) == (1.0, 0.0, 0.0, 1.0)
    with pytest.raises(ValueError):
        model.evaluate_generate(feats, labels, return_token_timestamps=True)
    with pytest.raises(TypeError):
        model.evaluate_generate(feats, labels.long())
    with pytest.raises(ValueError):
        model.evaluate_generate(feats, labels, torch.tensor([0, 0, 0]))


def test_evaluate_generate_whisper_is_the_sum_of_the_calls(setup):
    from tethys_speech_amd import train
    model, feats, labels, _ = setup
    lab = torch.from_numpy(labels)
    b1, b2 = (feats, lab), (feats.flip(0).contiguous(), lab[:, :5].contiguous())
    kw = dict(max_length=6, num_beams=2, num_return_sequences=2)
    lines = []
    total = train.evaluate_generate_whisper(None, model, [b1, b2], log=lines.append, step=3, **kw)
    r1, r2 = model.evaluate_generate(*b1, **kw), model.evaluate_generate(*b2, **kw)
    for k in COUNT_KEYS[:9]:
        assert total[k] == r1[k] + r2[k], k
    assert total["token_error_rate"] == total["n_edits"] / total["n_ref_tokens"]
    assert total["oracle_error_rate"] == total["n_oracle_edits"] / total["n_ref_tokens"]
    assert lines == [f"Eval step 3, TER: {total['token_error_rate']:.4f}, Sub: {int(total['n_sub'])}, "
                     f"Del: {int(total['n_del'])}, Ins: {int(total['n_ins'])}"]


def test_train_whisper_eval_generate_hook(dev):
    from tethys_speech_amd import dist, train
    from tethys_speech_amd.data import create_dummy_dataset
    data = dict(seq_len=96, max_target_length=12)
    tiny = dict(_TINY, n_ctx=64)

    def run(**kw):
        lines = []
        model = train.train_whisper(dist.DataParallelStrategy(0, 1), batch_size=3, num_batches=3, precision="bf16", device=dev,
                                    log=lines.append, model_overrides=tiny, eval_every=2, eval_batches=1, eval_seed=99, **data, **kw)
        return model, lines

    base, base_lines = run()
    assert not hasattr(base, "eval_generate_history") and not any("TER:" in l for l in base_lines)  # off by default
    model, lines = run(eval_generate=dict(max_length=5))
    assert model.losses == base.losses and [s for s, _ in model.eval_history] == [2, 3]
    hist = model.eval_generate_history
    assert [s for s, _ in hist] == [2, 3]
    kinds = [l.split(":")[0] for l in lines if l.startswith("Eval")]
    assert kinds == ["Eval step 2, Loss", "Eval step 2, TER", "Eval step 3, Loss", "Eval step 3, TER"]
    ds = iter(create_dummy_dataset(3, n_mels=16, device=dev, seed=99, **data))
    again = train.evaluate_generate_whisper(None, model, [next(ds)], max_length=5)
    assert again == hist[-1][1] and again["n_items"] == 3.0


def test_whisper_eval_job_generate_flag(dev, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "speech_jobs"))
    try:
        import whisper_eval
    finally:
        sys.path.pop(0)
    out = str(tmp_path / "eval.json")
    args = ["--model_type", "tiny", "--batch_size", "2", "--num_batches", "1", "--seq_len", "200", "--max_target_length", "6",
            "--seed", "5", "--out", out]
    whisper_eval.main(args)
    before = json.load(open(out))
    assert set(before) == {"model_type", "precision", "weights", "batch_size", "num_batches", "loss", "accuracy", "perplexity",
                           "n_tokens", "n_correct", "loss_sum", "seconds"}
    whisper_eval.main(args + ["--generate", "--num_beams", "2", "--nbest", "2", "--max_length", "4"])
    res = json.load(open(out))
    assert set(res) == set(before) | set(COUNT_KEYS) | {"generate", "generate_seconds"}
    assert all(res[k] == before[k] for k in before if k != "seconds")
    assert res["generate"] == {"num_beams": 2, "max_length": 4, "num_return_sequences": 2}
    assert res["n_items"] == 2.0 and 0.0 < res["n_ref_tokens"] <= 12.0 and res["n_sub"] + res["n_del"] + res["n_ins"] == res["n_edits"]
    assert res["token_error_rate"] == res["n_edits"] / res["n_ref_tokens"] and res["n_oracle_edits"] <= res["n_edits"]
    assert f"TER: {res['token_error_rate']:.4f}" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        whisper_eval.main(args + ["--num_beams", "2"])
