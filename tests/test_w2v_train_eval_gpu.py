"""The evaluation hooks of the Wav2Vec2 training loop, the evaluation job and the two-rank reduction on the GPU:
``train_wav2vec2(eval_every, eval_batches, eval_seed)`` on the reduced model - the Eval lines, where they fall among the step
lines, the history kept on the model, the same sets each time, and the step losses of the run without evaluation;
``speech_jobs/wav2vec2_eval.py`` end to end in a child process, with and without ``--ragged``; and
``train.evaluate_wav2vec2`` over two gloo ranks on the one GPU (fresh child processes, as tests/test_evaluate_two_rank_gpu.py)
against one process over the same batches."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from test_wav2vec2_gpu import small_cfg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP = 2600  # 130 frames on the reduced model


def _run(dev, **kw):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import dist, ops, train
    lines = []
    was = ops.set_deterministic(True)  # runs are compared with each other
    try:
        model = train.train_wav2vec2(dist.DataParallelStrategy(0, 1), model_size="base", batch_size=3, num_batches=5,
                                     precision="bf16", device=dev, log=lines.append, model_overrides=small_cfg(),
                                     clip_samples=CLIP, **kw)
    finally:
        ops.set_deterministic(was)
    return model, lines


def _step_part(line):
    return line.split(", Time:")[0]


def test_train_wav2vec2_eval_hooks(dev):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops, train, wav2vec2
    from tethys_speech_amd.data import W2VDummyDataset
    base, base_lines = _run(dev)
    base2, _ = _run(dev)
    assert not any(l.startswith("Eval") for l in base_lines) and not hasattr(base, "eval_history")
    model, lines = _run(dev, eval_every=2, eval_batches=2, eval_seed=99)
    # the step losses are those of the run without evaluation: exactly where two plain runs agree exactly (the Wav2Vec2
    # step keeps fp32 atomics: tests/test_plan_gpu.py), otherwise inside 4 x their spread
    assert len(model.losses) == 5 and len(base.losses) == 5
    spread = max(abs(a - b) for a, b in zip(base.losses, base2.losses))
    if spread == 0.0 and torch.equal(base.arena.p, base2.arena.p):
        print("plain runs agree bit for bit: comparing the run with evaluation bit for bit")
        assert model.losses == base.losses and torch.equal(model.arena.p, base.arena.p)
        assert [_step_part(l) for l in lines if not l.startswith("Eval")] == [_step_part(l) for l in base_lines]
    else:
        print(f"plain runs differ by {spread:.2e}: comparing within 4 x that spread")
        assert max(abs(a - b) for a, b in zip(model.losses, base.losses)) <= max(4.0 * spread, 1e-6 * abs(base.losses[0]))
    # every second step and once after the last; each Eval line follows the line of the step it was taken after
    kinds = [l.split(",")[0] for l in lines if l.startswith(("Step ", "Eval "))]
    assert kinds == ["Step 0", "Step 1", "Eval step 2", "Step 2", "Step 3", "Eval step 4", "Step 4", "Eval step 5"]
    hist = model.eval_history
    assert [s for s, _ in hist] == [2, 4, 5]
    evals = [l for l in lines if l.startswith("Eval")]
    G, Nc = model.config.num_codevector_groups, model.config.num_codevectors_per_group
    for (s, r), l in zip(hist, evals):
        assert l == f"Eval step {s}, Loss: {r['loss']:.4f}, Accuracy: {r['accuracy']:.4f}, Perplexity: {r['perplexity']:.4f}"
        assert r["n_frames"] == 2 * 3 * 130 and math.isfinite(r["loss"]) and 0.0 <= r["accuracy"] <= 1.0
        assert r["code_counts"].shape == (G, Nc) and r["code_counts"].sum(1).tolist() == [780, 780]
        assert r["perplexity"] == wav2vec2.perplexity_from_counts(r["code_counts"]) and 0.0 < r["code_usage"] <= 1.0
    assert len({r["loss"] for _, r in hist}) == 3  # (the weights moved between them)
    # every evaluation sees the same set, drawn once: the first two batches of the pool drawn with eval_seed and negatives
    # from default_rng(eval_seed + 1); the last evaluation again, directly, on the final weights
    ds = iter(W2VDummyDataset(3, length=CLIP, device=dev, seed=99))
    rng = np.random.default_rng(100)
    again_set = [(next(ds), torch.from_numpy(wav2vec2.sample_negative_indices(rng, 3, 130, model.config.num_negatives)).to(dev))
                 for _ in range(2)]
    was = ops.set_deterministic(True)
    try:
        again = train.evaluate_wav2vec2(None, model, again_set)
    finally:
        ops.set_deterministic(was)
    last = hist[-1][1]
    assert torch.equal(again["code_counts"], last["code_counts"])
    assert all(again[k] == last[k] for k in ("loss", "accuracy", "perplexity", "loss_sum", "n_correct", "n_frames"))
    # eval_every a divisor of the step count: no second evaluation at the end; one of the two left at 0: none at all
    m2, l2 = _run(dev, eval_every=5, eval_batches=1, eval_seed=99)
    assert [s for s, _ in m2.eval_history] == [5] and sum(l.startswith("Eval") for l in l2) == 1
    assert m2.eval_history[0][1]["n_frames"] == 3 * 130
    m3, l3 = _run(dev, eval_every=2, eval_batches=0)
    assert not any(l.startswith("Eval") for l in l3) and not hasattr(m3, "eval_history")
    with pytest.raises(ValueError):
        _run(dev, eval_every=2, eval_batches=1, eval_seed=1234)  # the training pool's own seed


@pytest.mark.parametrize("ragged", [False, True], ids=["padded", "ragged"])
def test_wav2vec2_eval_job(dev, tmp_path, ragged):
    """The CLI end to end in a child process, on the smallest built-in size."""
    out = str(tmp_path / "eval.json")
    args = [sys.executable, os.path.join(ROOT, "speech_jobs", "wav2vec2_eval.py"), "--model_size", "tiny", "--batch_size", "3",
            "--num_batches", "2", "--clip_samples", "4000", "--seed", "5", "--out", out] + (["--ragged"] if ragged else [])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run(args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.load(open(out))
    assert res["ragged"] is ragged and res["model_size"] == "tiny" and res["precision"] == "bf16"
    line = (f"Loss: {res['loss']:.4f}, Accuracy: {res['accuracy']:.4f}, Perplexity: {res['perplexity']:.4f}, "
            f"Code usage: {res['code_usage']:.4f}")
    assert line in p.stdout
    T = 100  # 4000 samples through the tiny stem's strides 5 * 2 * 2 * 2
    if ragged:
        assert 2 * 3 * T / 4 <= res["n_frames"] < 2 * 3 * T
    else:
        assert res["n_frames"] == 2 * 3 * T
    assert all(math.isfinite(res[k]) for k in ("loss", "contrastive_loss", "accuracy", "perplexity", "code_usage", "loss_sum"))
    assert 0.0 <= res["accuracy"] <= 1.0 and 0.0 < res["code_usage"] <= 1.0 and res["perplexity"] >= 1.0
    assert abs(res["loss"] - (res["contrastive_loss"] - 0.1 * res["perplexity"])) < 1e-12


# ----------------------------------------------------------------------------- two ranks
def _batches():
    """Three global batches of 4 clips with their negatives (T = 85 frames); ranks take rows [0, 2) and [2, 4)."""
    from tethys_speech_amd import wav2vec2
    rng = np.random.default_rng(17)
    out = []
    for _ in range(3):
        audio = rng.standard_normal((4, 1700)).astype(np.float32)
        out.append((audio, wav2vec2.sample_negative_indices(rng, 4, 85, small_cfg()["num_negatives"])))
    return out


def _shard(rank):
    return [(a[2 * rank:2 * rank + 2], n[2 * rank:2 * rank + 2]) for a, n in _batches()]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import dist as D, ops, train, wav2vec2
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = "cuda:0"
    strat = D.DataParallelStrategy(rank, 2, backend="gloo")
    model = wav2vec2.create_full_model("pretraining", "base", device=dev, precision="fp32", seed=11 + rank, **small_cfg())
    strat.broadcast_parameters(model.arena.p)
    model.refresh_shadows()
    ops.set_deterministic(True)
    calls, real = [0], dist.all_reduce

    def counted(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)
    dist.all_reduce = counted
    lines = []
    data = [(torch.from_numpy(a).to(dev), torch.from_numpy(n).to(dev)) for a, n in _shard(rank)]
    out = train.evaluate_wav2vec2(strat, model, data, log=lines.append, step=7)
    dist.all_reduce = real
    torch.cuda.synchronize()
    out["code_counts"] = out["code_counts"].tolist()
    q.put((rank, out, calls[0], lines))
    dist.destroy_process_group()


def test_two_rank_evaluation_equals_one_process_over_the_same_batches(dev):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(2)]
    for p_ in procs:
        p_.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda t: t[0])
    for p_ in procs:
        p_.join(60)
    (_, o0, c0, lines0), (_, o1, c1, _) = res
    assert o0 == o1, "the ranks disagree on the reduced result"
    assert c0 == 1 and c1 == 1, "one all-reduce after the loop, none per batch"

    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops, train, wav2vec2
    model = wav2vec2.create_full_model("pretraining", "base", device=dev, precision="fp32", seed=11, **small_cfg())
    # the same batches in the same shapes (a GEMM may pick another tile for another row count: same clips, other bits)
    union = [(torch.from_numpy(a).to(dev), torch.from_numpy(n).to(dev)) for r in range(2) for a, n in _shard(r)]
    was = ops.set_deterministic(True)
    try:
        ref = train.evaluate_wav2vec2(None, model, union)
    finally:
        ops.set_deterministic(was)
    assert o0["n_frames"] == ref["n_frames"] == 3 * 4 * 85 and o0["n_correct"] == ref["n_correct"]
    assert o0["code_counts"] == ref["code_counts"].tolist()
    assert o0["perplexity"] == ref["perplexity"] and o0["code_usage"] == ref["code_usage"]
    # the same fp32 row losses, added in another order in fp64: a few ulp of the sum
    assert abs(o0["loss_sum"] - ref["loss_sum"]) <= 1e-12 * abs(ref["loss_sum"])
    assert abs(o0["loss"] - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    assert lines0 == [f"Eval step 7, Loss: {o0['loss']:.4f}, Accuracy: {o0['accuracy']:.4f}, Perplexity: {o0['perplexity']:.4f}"]
