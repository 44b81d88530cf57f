"""The evaluation hooks of the training loop and the evaluation job on the GPU: ``train_whisper(eval_every, eval_batches,
eval_seed)`` on the tiny model of the training-loop tests - the Eval lines, where they fall among the step lines, the
history kept on the model, and training itself unchanged to the bit - and ``speech_jobs/whisper_eval.py`` run in-process
against a direct ``evaluate_whisper`` of the same weights and pool."""
import json
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TINY = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, vocab_size=160, encoder_layers=2,
             decoder_layers=2, n_mels=16, n_ctx=64, decoder_start_token_id=150, max_target_positions=32)
_DATA = dict(seq_len=96, max_target_length=12)


def _run(dev, **kw):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import dist, ops, train
    lines = []
    was = ops.set_deterministic(True)  # two runs are compared to the bit
    try:
        model = train.train_whisper(dist.DataParallelStrategy(0, 1), batch_size=3, num_batches=5, precision="bf16", device=dev,
                                    log=lines.append, model_overrides=_TINY, **_DATA, **kw)
    finally:
        ops.set_deterministic(was)
    return model, lines


def _step_part(line):
    return line.split(", Time:")[0]  # "Step i, Loss: x.xxxx" (the rest of the line is the wall clock)


def test_train_whisper_eval_hooks(dev):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import train
    from tethys_speech_amd.data import create_dummy_dataset
    base, base_lines = _run(dev)
    assert not any(l.startswith("Eval") for l in base_lines) and not hasattr(base, "eval_history")
    model, lines = _run(dev, eval_every=2, eval_batches=1, eval_seed=99)
    # training is untouched to the bit: the same losses, the same parameters, the same lines apart from the Eval lines
    assert model.losses == base.losses and len(model.losses) == 5
    assert torch.equal(model.arena.p, base.arena.p) and torch.equal(model.arena.m, base.arena.m)
    assert [_step_part(l) for l in lines if not l.startswith("Eval")] == [_step_part(l) for l in base_lines]
    # every second step and once after the last; each Eval line follows the line of the step it was taken after
    kinds = [l.split(",")[0] for l in lines if l.startswith(("Step ", "Eval "))]
    assert kinds == ["Step 0", "Step 1", "Eval step 2", "Step 2", "Step 3", "Eval step 4", "Step 4", "Eval step 5"]
    hist = model.eval_history
    assert [s for s, _ in hist] == [2, 4, 5]
    evals = [l for l in lines if l.startswith("Eval")]
    for (s, r), l in zip(hist, evals):
        assert l == f"Eval step {s}, Loss: {r['loss']:.4f}, Accuracy: {r['accuracy']:.4f}"
        assert r["n_tokens"] == 3 * 11 and math.isfinite(r["loss"]) and 0.0 <= r["accuracy"] <= 1.0
    assert len({r["loss"] for _, r in hist}) == 3  # (the weights moved between them)
    # every evaluation sees the first batch of the pool drawn with eval_seed: the last one again, directly, on the final weights
    ds = iter(create_dummy_dataset(3, n_mels=16, device=dev, seed=99, **_DATA))
    again = train.evaluate_whisper(None, model, [next(ds)])
    assert again == hist[-1][1]
    other = train.evaluate_whisper(None, model, [next(ds)])
    assert other["loss"] != again["loss"]
    # eval_every a divisor of the step count: no second evaluation at the end; one of the two left at 0: none at all
    m2, l2 = _run(dev, eval_every=5, eval_batches=2, eval_seed=99)
    assert [s for s, _ in m2.eval_history] == [5] and sum(l.startswith("Eval") for l in l2) == 1
    assert m2.eval_history[0][1]["n_tokens"] == 2 * 3 * 11 and m2.losses == base.losses
    m3, l3 = _run(dev, eval_every=2, eval_batches=0)
    assert not any(l.startswith("Eval") for l in l3) and not hasattr(m3, "eval_history")
    with pytest.raises(ValueError):
        _run(dev, eval_every=2, eval_batches=1, eval_seed=1234)  # the training pool's own seed


def test_whisper_eval_job(dev, tmp_path, capsys):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import train, whisper
    from tethys_speech_amd.data import create_dummy_dataset
    sys.path.insert(0, os.path.join(ROOT, "speech_jobs"))
    try:
        import whisper_eval
    finally:
        sys.path.pop(0)
    src = whisper.create_whisper_model("tiny", device=dev, precision="bf16", seed=77)  # not the job's own initialisation
    wpath, out = str(tmp_path / "w.pt"), str(tmp_path / "eval.json")
    train.save_weights(src, wpath)
    args = ["--model_type", "tiny", "--batch_size", "2", "--num_batches", "2", "--seq_len", "200", "--max_target_length", "6",
            "--seed", "5", "--out", out]
    whisper_eval.main(args + ["--weights", wpath])
    res = json.load(open(out))
    ds = iter(create_dummy_dataset(2, n_mels=80, seq_len=200, max_target_length=6, device=dev, seed=5))
    ref = train.evaluate_whisper(None, src, [next(ds), next(ds)])
    assert all(res[k] == ref[k] for k in ("loss", "accuracy", "loss_sum", "n_correct", "n_tokens")) and res["n_tokens"] == 20
    assert res["perplexity"] == math.exp(res["loss"]) and res["weights"] == wpath and res["precision"] == "bf16"
    printed = capsys.readouterr().out
    assert f"Loss: {res['loss']:.4f}, Accuracy: {res['accuracy']:.4f}, Perplexity: {res['perplexity']:.4f}" in printed
    # without --weights the job scores its own seeded initialisation: other weights, another loss
    whisper_eval.main(args)
    assert json.load(open(out))["loss"] != res["loss"]
    with pytest.raises(SystemExit):
        whisper_eval.main(["--num_batches", "0"])
